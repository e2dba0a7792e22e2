// vg_corners_tu.hip -- translation unit of libvisgeom_amd.so: checkerboard corner detection (section 8 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_corner_detector owns the device scratch and the pinned host staging of one image size.  A detect call works through its
// images in chunks of at most `chunk` images (device scratch <= kCornerDeviceBudget, see the header); every chunk runs the
// reference's sigma retries {1.4, 2, 1} (detectPattern .cpp:223-260), each pass batched over the images still not found.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "vg_corners.hpp"
#include "vg_corners_graph.hpp"
#include "vg_host_parallel.hpp"
#include "vg_internal.hpp"

namespace {

using vgi::fail;

constexpr int64_t kCornerDeviceBudget = int64_t(1) << 30;   // device scratch of one detector, bytes (one image more if it is larger)
constexpr int kCornerMaxChunk = 64;
constexpr int kGraphThreads = 16;                           // host threads of the graph stage
const double kSigmas[3] = {1.4, 2., 1.};

// cv::getGaussianKernel(n, sigma, CV_64F) for sigma > 0: exp(-x^2 / (2 sigma^2)) normalised to sum 1, then rounded to float
void gaussian(int n, double sigma, float *w)
{
    std::vector<double> cf(n);
    const double scale2X = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < n; i++) {
        const double x = i - (n - 1) * 0.5;
        cf[i] = std::exp(scale2X * x * x);
        sum += cf[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) w[i] = (float)(cf[i] * sum);
}

vg::BlurWeights blur_weights(double sigma)
{
    vg::BlurWeights b{};
    gaussian(3, 0.7, b.w1);
    b.r2 = (int)std::ceil(sigma);
    gaussian(2 * b.r2 + 1, sigma, b.w2);
    return b;
}

bool valid_sigma(double s) { return s == 1.4 || s == 2. || s == 1.; }
int init_radius(double sigma) { return (int)std::round(1.5 * sigma); }   // detectPattern .cpp:232

template <class T>
T *carve(char *&p, size_t n)
{
    T *r = reinterpret_cast<T *>(p);
    p += (n * sizeof(T) + 255) & ~size_t(255);
    return r;
}
template <class T>
size_t carve_size(size_t n) { return (n * sizeof(T) + 255) & ~size_t(255); }

}  // namespace

struct vg_corner_detector {
    int device = 0;
    hipStream_t stream = nullptr;
    int Nx = 0, Ny = 0;
    bool improve = false;
    vg::CircleTable ct{};
    // sized for (W, H, chunk)
    int W = 0, H = 0, chunk = 0, tiles_x = 0, tiles = 0;
    int64_t cap = 0;
    size_t plane = 0;
    vgi::DeviceMem<char> dev;
    int64_t *d_list = nullptr;
    uint8_t *d_src2 = nullptr;
    float *d_gx = nullptr, *d_gy = nullptr, *d_imgrad = nullptr, *d_resp = nullptr;
    double *d_psum = nullptr, *d_avg = nullptr, *d_thresh = nullptr, *d_gthresh = nullptr;
    int *d_pcnt = nullptr, *d_counts = nullptr;   // [4][chunk]: maxima, accepted, top-K, hypotheses
    uint64_t *d_keys = nullptr, *d_acc = nullptr, *d_sel = nullptr, *d_hyp = nullptr;
    int *d_trans = nullptr;
    double *d_rinit = nullptr, *d_rprior = nullptr, *d_rrad = nullptr, *d_rout = nullptr;
    int *d_rslot = nullptr;
    vgi::PinnedMem<char> host;
    int64_t *h_list = nullptr;
    uint8_t *h_src2 = nullptr;
    float *h_gx = nullptr, *h_gy = nullptr;
    int *h_counts = nullptr, *h_trans = nullptr, *h_rslot = nullptr;
    double *h_gthresh = nullptr, *h_rinit = nullptr, *h_rprior = nullptr, *h_rrad = nullptr, *h_rout = nullptr;
    double stats[8] = {0};   // gpu_s, d2h_s, d2h_bytes, graph_s, graph_images, refine_s, refine_corners, calls

    int n_corners() const { return Nx * Ny; }
    int max_hyp() const { return 10 * Nx * Ny; }   // MAX_CANDIDATE_COUNT

    static size_t device_bytes(int W, int H, int chunk, int64_t cap, int tiles, int nc)
    {
        const size_t plane = (size_t)W * H, c = (size_t)chunk;
        return carve_size<int64_t>(c) + carve_size<uint8_t>(c * plane) + 4 * carve_size<float>(c * plane) +
               carve_size<double>(c * tiles) + carve_size<int>(c * tiles) + 2 * carve_size<double>(c) + carve_size<int>(4 * c) +
               2 * carve_size<uint64_t>(c * cap) + 2 * carve_size<uint64_t>(c * vg::kSelectMax) +
               carve_size<int>(c * vg::kSelectMax * 9) + carve_size<double>(c * vg::kSelectMax) + carve_size<double>(c * nc * 5) +
               2 * carve_size<double>(c * nc * 2) + carve_size<double>(c * nc) + carve_size<int>(c * nc);
    }
    static size_t host_bytes(int W, int H, int chunk, int nc)
    {
        const size_t plane = (size_t)W * H, c = (size_t)chunk;
        return carve_size<int64_t>(c) + carve_size<uint8_t>(c * plane) + 2 * carve_size<float>(c * plane) + carve_size<int>(4 * c) +
               carve_size<int>(c * vg::kSelectMax * 9) + carve_size<double>(c * vg::kSelectMax) + carve_size<int>(c * nc) +
               carve_size<double>(c * nc * 5) + 2 * carve_size<double>(c * nc * 2) + carve_size<double>(c * nc);
    }

    int ensure(int w, int h)
    {
        if (w == W && h == H && dev) return VG_OK;
        (void)dev.release();
        (void)host.release();
        W = H = chunk = 0;
        const int tx = (w + vg::kCornerTileW - 1) / vg::kCornerTileW, ty = (h + vg::kCornerTileH - 1) / vg::kCornerTileH;
        const int64_t cp = (int64_t)((w + 1) / 2) * ((h + 1) / 2);
        const int nc = n_corners();
        int c = kCornerMaxChunk;
        while (c > 1 && device_bytes(w, h, c, cp, tx * ty, nc) > (size_t)kCornerDeviceBudget) c--;
        VG_HIP(hipSetDevice(device));
        vgi::DeviceMem<char> d;
        vgi::PinnedMem<char> hp;
        if (d.alloc(device_bytes(w, h, c, cp, tx * ty, nc)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(VG_ERR_ALLOC, "corner detector: device scratch allocation failed");
        }
        if (hp.alloc(host_bytes(w, h, c, nc), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return fail(VG_ERR_ALLOC, "corner detector: pinned host allocation failed");
        }
        dev = std::move(d);
        host = std::move(hp);
        W = w;
        H = h;
        chunk = c;
        tiles_x = tx;
        tiles = tx * ty;
        cap = cp;
        plane = (size_t)w * h;
        const size_t C = (size_t)c;
        char *p = dev;
        d_list = carve<int64_t>(p, C);
        d_src2 = carve<uint8_t>(p, C * plane);
        d_gx = carve<float>(p, C * plane);
        d_gy = carve<float>(p, C * plane);
        d_imgrad = carve<float>(p, C * plane);
        d_resp = carve<float>(p, C * plane);
        d_psum = carve<double>(p, C * tiles);
        d_pcnt = carve<int>(p, C * tiles);
        d_avg = carve<double>(p, C);
        d_thresh = carve<double>(p, C);
        d_counts = carve<int>(p, 4 * C);
        d_keys = carve<uint64_t>(p, C * cap);
        d_acc = carve<uint64_t>(p, C * cap);
        d_sel = carve<uint64_t>(p, C * vg::kSelectMax);
        d_hyp = carve<uint64_t>(p, C * vg::kSelectMax);
        d_trans = carve<int>(p, C * vg::kSelectMax * 9);
        d_gthresh = carve<double>(p, C * vg::kSelectMax);
        d_rinit = carve<double>(p, C * nc * 5);
        d_rprior = carve<double>(p, C * nc * 2);
        d_rout = carve<double>(p, C * nc * 2);
        d_rrad = carve<double>(p, C * nc);
        d_rslot = carve<int>(p, C * nc);
        char *q = host;
        h_list = carve<int64_t>(q, C);
        h_src2 = carve<uint8_t>(q, C * plane);
        h_gx = carve<float>(q, C * plane);
        h_gy = carve<float>(q, C * plane);
        h_counts = carve<int>(q, 4 * C);
        h_trans = carve<int>(q, C * vg::kSelectMax * 9);
        h_gthresh = carve<double>(q, C * vg::kSelectMax);
        h_rslot = carve<int>(q, C * nc);
        h_rinit = carve<double>(q, C * nc * 5);
        h_rprior = carve<double>(q, C * nc * 2);
        h_rout = carve<double>(q, C * nc * 2);
        h_rrad = carve<double>(q, C * nc);
        return VG_OK;
    }

    // stages 1-3 on `ns` slots; h_list[0..ns) already holds the images.  Maps go to the given planes (scratch by default).
    int response(const uint8_t *images, int ns, double sigma, uint8_t *src1, uint8_t *src2, float *gx, float *gy, float *ig, float *rs)
    {
        VG_HIP(hipMemcpyAsync(d_list, h_list, sizeof(int64_t) * ns, hipMemcpyHostToDevice, stream));
        vg::ResponseArgs a;
        a.images = images;
        a.list = d_list;
        a.W = W;
        a.H = H;
        a.tiles_x = tiles_x;
        a.tiles_per_image = tiles;
        a.bw = blur_weights(sigma);
        a.src1 = src1;
        a.src2 = src2;
        a.gradx = gx;
        a.grady = gy;
        a.imgrad = ig;
        a.resp = rs;
        a.part_sum = d_psum;
        a.part_cnt = d_pcnt;
        hipLaunchKernelGGL(vg::vg_corner_response_kernel, dim3(tiles, ns), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(vg::vg_corner_mean_kernel, dim3(ns), dim3(256), 0, stream, (const double *)d_psum, (const int *)d_pcnt, tiles,
                           d_avg);
        VG_HIP(hipGetLastError());
        return VG_OK;
    }

    // stages 1-6 into the scratch
    int candidates(const uint8_t *images, int ns, double sigma)
    {
        VG_HIP(hipMemsetAsync(d_counts, 0, sizeof(int) * 4 * chunk, stream));
        if (int rc = response(images, ns, sigma, nullptr, d_src2, d_gx, d_gy, d_imgrad, d_resp)) return rc;
        const int R = init_radius(sigma);
        vg::MaximaArgs m;
        m.resp = d_resp;
        m.avg = d_avg;
        m.W = W;
        m.H = H;
        m.tiles_x = tiles_x;
        m.radius = R;
        m.keys = d_keys;
        m.count = d_counts;
        m.cap = cap;
        hipLaunchKernelGGL(vg::vg_corner_maxima_kernel, dim3(tiles, ns), dim3(256), 0, stream, m);
        vg::SelectArgs s;
        s.keys = d_keys;
        s.count = d_counts;
        s.cap = cap;
        s.M = n_corners();
        s.ref_count = n_corners();
        s.out = d_sel;
        s.out_count = d_counts + 2 * chunk;
        s.thresh = d_thresh;
        hipLaunchKernelGGL(vg::vg_corner_select_kernel, dim3(ns), dim3(vg::kSelectThreads), 0, stream, s);
        vg::CheckArgs c;
        c.images = images;
        c.list = d_list;
        c.gradx = d_gx;
        c.grady = d_gy;
        c.W = W;
        c.H = H;
        c.init_radius = R;
        c.keys = d_keys;
        c.count = d_counts;
        c.thresh = d_thresh;
        c.cap = cap;
        c.ct = ct;
        c.acc_keys = d_acc;
        c.acc_count = d_counts + chunk;
        hipLaunchKernelGGL(vg::vg_corner_check_kernel, dim3(64, ns), dim3(vg::kCheckLanes), 0, stream, c);
        s.keys = d_acc;
        s.count = d_counts + chunk;
        s.M = max_hyp();
        s.ref_count = 0;
        s.out = d_hyp;
        s.out_count = d_counts + 3 * chunk;
        s.thresh = nullptr;
        hipLaunchKernelGGL(vg::vg_corner_select_kernel, dim3(ns), dim3(vg::kSelectThreads), 0, stream, s);
        vg::TransitionArgs t;
        t.images = images;
        t.list = d_list;
        t.imgrad = d_imgrad;
        t.W = W;
        t.H = H;
        t.init_radius = R;
        t.hyp = d_hyp;
        t.hyp_count = d_counts + 3 * chunk;
        t.ct = ct;
        t.trans = d_trans;
        t.grad_thresh = d_gthresh;
        hipLaunchKernelGGL(vg::vg_corner_transitions_kernel, dim3((max_hyp() + vg::kCheckLanes - 1) / vg::kCheckLanes, ns),
                           dim3(vg::kCheckLanes), 0, stream, t);
        VG_HIP(hipGetLastError());
        return VG_OK;
    }

    // the whole detection of images [0, n): corners HOST [n][Nx Ny][2], found [n], sigma_out [n] or nullptr
    int detect(int64_t n, const uint8_t *images, double *corners, uint8_t *found, double *sigma_out)
    {
        using clk = std::chrono::steady_clock;
        auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
        const int nc = n_corners();
        stats[7] += 1;
        for (int64_t i = 0; i < n; i++) {
            found[i] = 0;
            if (sigma_out) sigma_out[i] = 0.;
            std::fill(corners + (size_t)i * nc * 2, corners + (size_t)(i + 1) * nc * 2, 0.);
        }
        for (int64_t c0 = 0; c0 < n; c0 += chunk) {
            std::vector<int64_t> pending;
            for (int64_t i = c0; i < std::min(n, c0 + (int64_t)chunk); i++) pending.push_back(i);
            for (int si = 0; si < 3 && !pending.empty(); si++) {
                const double sigma = kSigmas[si];
                const int ns = (int)pending.size();
                const clk::time_point t0 = clk::now();
                for (int s = 0; s < ns; s++) h_list[s] = pending[s];
                if (int rc = candidates(images, ns, sigma)) return rc;
                VG_HIP(hipMemcpyAsync(h_counts, d_counts, sizeof(int) * 4 * chunk, hipMemcpyDeviceToHost, stream));
                VG_HIP(hipStreamSynchronize(stream));
                const clk::time_point t1 = clk::now();
                stats[0] += secs(t0, t1);
                // .cpp:236: fewer hypotheses than corners -> the next sigma.  Only the images that go on to the graph stage
                // come back to the host, and of them only what that stage reads.
                std::vector<int> live;
                double bytes = 0;
                for (int s = 0; s < ns; s++) {
                    const int nh = h_counts[3 * chunk + s];
                    if (nh < nc) continue;
                    live.push_back(s);
                    const size_t o = (size_t)s * plane;
                    VG_HIP(hipMemcpyAsync(h_src2 + o, d_src2 + o, plane, hipMemcpyDeviceToHost, stream));
                    VG_HIP(hipMemcpyAsync(h_gx + o, d_gx + o, plane * 4, hipMemcpyDeviceToHost, stream));
                    VG_HIP(hipMemcpyAsync(h_gy + o, d_gy + o, plane * 4, hipMemcpyDeviceToHost, stream));
                    const size_t ho = (size_t)s * vg::kSelectMax;
                    VG_HIP(hipMemcpyAsync(h_trans + ho * 9, d_trans + ho * 9, sizeof(int) * 9 * nh, hipMemcpyDeviceToHost, stream));
                    VG_HIP(hipMemcpyAsync(h_gthresh + ho, d_gthresh + ho, sizeof(double) * nh, hipMemcpyDeviceToHost, stream));
                    bytes += plane * 9. + nh * 44.;
                }
                VG_HIP(hipStreamSynchronize(stream));
                const clk::time_point t2 = clk::now();
                stats[1] += secs(t1, t2);
                stats[2] += bytes;
                // the graph stages, one image per task on at most 16 host threads
                std::vector<std::vector<int>> pattern(live.size());   // per live slot: hypothesis index of every corner, or empty
                std::atomic<size_t> next(0);
                const int nthreads = std::max(1, std::min({kGraphThreads, vgpar::host_threads(), (int)live.size()}));
                vgpar::parallel_ranges((size_t)nthreads, 1, [&](size_t, size_t, int) {
                    for (size_t k; (k = next.fetch_add(1)) < live.size();) {
                        const int s = live[k];
                        vgcorner::ImageView im;
                        im.W = W;
                        im.H = H;
                        im.init_radius = init_radius(sigma);
                        im.src2 = h_src2 + (size_t)s * plane;
                        im.gradx = h_gx + (size_t)s * plane;
                        im.grady = h_gy + (size_t)s * plane;
                        im.n_hyp = h_counts[3 * chunk + s];
                        im.trans = h_trans + (size_t)s * vg::kSelectMax * 9;
                        im.grad_thresh = h_gthresh + (size_t)s * vg::kSelectMax;
                        vgcorner::Graph g(im, Nx, Ny);
                        g.construct();
                        const std::vector<int> idx = g.select_pattern();
                        if ((int)idx.size() == nc)
                            for (int id : idx) pattern[k].push_back(g.hyp_of(id));
                    }
                });
                const clk::time_point t3 = clk::now();
                stats[3] += secs(t2, t3);
                stats[4] += (double)live.size();
                // corners of the images found at this sigma; improveCorners on the GPU for all of them at once
                std::vector<int64_t> next_pending;
                std::vector<char> done(ns, 0);
                int64_t nr = 0;
                for (size_t k = 0; k < live.size(); k++) {
                    if (pattern[k].empty()) continue;
                    const int s = live[k];
                    done[s] = 1;
                    const int64_t img = pending[s];
                    const int *tr = h_trans + (size_t)s * vg::kSelectMax * 9;
                    std::vector<double> pts(2 * nc);
                    for (int j = 0; j < nc; j++) {
                        pts[2 * j] = tr[9 * pattern[k][j]];
                        pts[2 * j + 1] = tr[9 * pattern[k][j] + 1];
                    }
                    std::copy(pts.begin(), pts.end(), corners + (size_t)img * nc * 2);
                    found[img] = 1;
                    if (sigma_out) sigma_out[img] = sigma;
                    if (!improve) continue;
                    std::vector<double> rad;
                    vgcorner::refine_radii(pts, Nx, rad);
                    for (int j = 0; j < nc; j++) {
                        double init[5];
                        if (!vgcorner::init_point(tr + 9 * pattern[k][j], init)) continue;   // left unrefined
                        h_rslot[nr] = s;
                        std::copy(init, init + 5, h_rinit + 5 * nr);
                        h_rprior[2 * nr] = pts[2 * j];
                        h_rprior[2 * nr + 1] = pts[2 * j + 1];
                        h_rrad[nr] = rad[j];
                        h_rout[2 * nr] = (double)img;   // where the result goes (host side only)
                        h_rout[2 * nr + 1] = (double)j;
                        nr++;
                    }
                }
                if (nr > 0) {
                    std::vector<int64_t> dst(nr);
                    for (int64_t r = 0; r < nr; r++) dst[r] = (int64_t)h_rout[2 * r] * nc + (int64_t)h_rout[2 * r + 1];
                    VG_HIP(hipMemcpyAsync(d_rslot, h_rslot, sizeof(int) * nr, hipMemcpyHostToDevice, stream));
                    VG_HIP(hipMemcpyAsync(d_rinit, h_rinit, sizeof(double) * 5 * nr, hipMemcpyHostToDevice, stream));
                    VG_HIP(hipMemcpyAsync(d_rprior, h_rprior, sizeof(double) * 2 * nr, hipMemcpyHostToDevice, stream));
                    VG_HIP(hipMemcpyAsync(d_rrad, h_rrad, sizeof(double) * nr, hipMemcpyHostToDevice, stream));
                    vg::RefineArgs r;
                    r.gradx = d_gx;
                    r.grady = d_gy;
                    r.W = W;
                    r.H = H;
                    r.n = nr;
                    r.slot = d_rslot;
                    r.init = d_rinit;
                    r.prior = d_rprior;
                    r.radius = d_rrad;
                    r.out = d_rout;
                    hipLaunchKernelGGL(vg::vg_corner_refine_kernel, dim3((unsigned)((nr + 63) / 64)), dim3(64), 0, stream, r);
                    VG_HIP(hipGetLastError());
                    VG_HIP(hipMemcpyAsync(h_rout, d_rout, sizeof(double) * 2 * nr, hipMemcpyDeviceToHost, stream));
                    VG_HIP(hipStreamSynchronize(stream));
                    for (int64_t q = 0; q < nr; q++) {
                        corners[2 * dst[q]] = h_rout[2 * q];
                        corners[2 * dst[q] + 1] = h_rout[2 * q + 1];
                    }
                    stats[5] += secs(t3, clk::now());
                    stats[6] += (double)nr;
                }
                for (int s = 0; s < ns; s++)
                    if (!done[s]) next_pending.push_back(pending[s]);
                pending.swap(next_pending);
            }
        }
        return VG_OK;
    }
};

namespace {

int check_images(const vg_corner_detector *d, int64_t n, int w, int h, const void *images)
{
    if (!d) return fail(VG_ERR_INVALID_ARGUMENT, "NULL detector");
    if (n < 0) return fail(VG_ERR_INVALID_ARGUMENT, "negative image count");
    if (w < vg::kCornerMinDim || h < vg::kCornerMinDim || w > vg::kCornerMaxDim || h > vg::kCornerMaxDim)
        return fail(VG_ERR_INVALID_ARGUMENT, "image sides must be in [16, 16384]");
    if (n > 0 && !images) return fail(VG_ERR_INVALID_ARGUMENT, "NULL images");
    return VG_OK;
}

}  // namespace

extern "C" {

int vg_corner_circle(int radius, int max_points, int32_t *du, int32_t *dv, int *n_points)
{
    if (radius < 1 || radius > 64) return fail(VG_ERR_INVALID_ARGUMENT, "radius must be in [1, 64]");
    if (!du || !dv || !n_points || max_points < 0) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    const auto c = vgcorner::raster_circle(radius);
    for (size_t i = 0; i < c.size() && (int)i < max_points; i++) {
        du[i] = c[i][0];
        dv[i] = c[i][1];
    }
    *n_points = (int)c.size();
    return VG_OK;
}

int vg_corner_detector_create(vg_corner_detector **out, int device, void *hip_stream, int cols, int rows, int improve)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (cols < 2 || rows < 2 || cols * rows > 400)
        return fail(VG_ERR_INVALID_ARGUMENT, "the board needs cols, rows >= 2 and at most 400 corners");
    if (improve != 0 && improve != 1) return fail(VG_ERR_INVALID_ARGUMENT, "improve must be 0 or 1");
    if (const int rc = vgi::check_device(device, "corner detection")) return rc;
    vg_corner_detector *d = new (std::nothrow) vg_corner_detector();
    if (!d) return fail(VG_ERR_ALLOC, "out of host memory");
    d->device = device;
    d->stream = reinterpret_cast<hipStream_t>(hip_stream);
    d->Nx = cols;
    d->Ny = rows;
    d->improve = improve != 0;
    d->ct = vgcorner::circle_table();
    *out = d;
    return VG_OK;
}

void vg_corner_detector_destroy(vg_corner_detector *d)
{
    if (!d) return;
    (void)hipSetDevice(d->device);
    (void)hipStreamSynchronize(d->stream);
    delete d;
}

int vg_corner_detect(vg_corner_detector *d, int64_t n_images, int width, int height, const uint8_t *images, double *corners,
                     uint8_t *found, double *sigma)
{
    if (const int rc = check_images(d, n_images, width, height, images)) return rc;
    if (n_images > 0 && (!corners || !found)) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    if (n_images == 0) return VG_OK;
    VG_HIP(hipSetDevice(d->device));
    if (const int rc = d->ensure(width, height)) return rc;
    return d->detect(n_images, images, corners, found, sigma);
}

int vg_corner_response(vg_corner_detector *d, int64_t n_images, int width, int height, const uint8_t *images, double sigma,
                       uint8_t *src1, uint8_t *src2, float *gradx, float *grady, float *imgrad, float *resp, double *avg)
{
    if (const int rc = check_images(d, n_images, width, height, images)) return rc;
    if (!valid_sigma(sigma)) return fail(VG_ERR_INVALID_ARGUMENT, "sigma must be one of the detector's 1.4, 2, 1");
    if (n_images > 0 && (!src1 || !src2 || !gradx || !grady || !imgrad || !resp || !avg))
        return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    if (n_images == 0) return VG_OK;
    VG_HIP(hipSetDevice(d->device));
    if (const int rc = d->ensure(width, height)) return rc;
    const size_t plane = d->plane;
    for (int64_t c0 = 0; c0 < n_images; c0 += d->chunk) {
        const int ns = (int)std::min<int64_t>(d->chunk, n_images - c0);
        for (int s = 0; s < ns; s++) d->h_list[s] = s;
        const size_t o = (size_t)c0 * plane;
        if (int rc = d->response(images + o, ns, sigma, src1 + o, src2 + o, gradx + o, grady + o, imgrad + o, resp + o)) return rc;
        VG_HIP(hipMemcpyAsync(avg + c0, d->d_avg, sizeof(double) * ns, hipMemcpyDeviceToHost, d->stream));
        VG_HIP(hipStreamSynchronize(d->stream));
    }
    return VG_OK;
}

int vg_corner_candidates(vg_corner_detector *d, int64_t n_images, int width, int height, const uint8_t *images, double sigma,
                         int max_out, int32_t *uv, int32_t *count, double *val_thresh, int64_t *n_maxima)
{
    if (const int rc = check_images(d, n_images, width, height, images)) return rc;
    if (!valid_sigma(sigma)) return fail(VG_ERR_INVALID_ARGUMENT, "sigma must be one of the detector's 1.4, 2, 1");
    if (max_out < 0) return fail(VG_ERR_INVALID_ARGUMENT, "negative max_out");
    if (n_images > 0 && (!uv || !count || !val_thresh || !n_maxima)) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    if (n_images == 0) return VG_OK;
    VG_HIP(hipSetDevice(d->device));
    if (const int rc = d->ensure(width, height)) return rc;
    std::vector<uint64_t> keys(vg::kSelectMax);
    std::vector<double> th(d->chunk);
    for (int64_t c0 = 0; c0 < n_images; c0 += d->chunk) {
        const int ns = (int)std::min<int64_t>(d->chunk, n_images - c0);
        for (int s = 0; s < ns; s++) d->h_list[s] = c0 + s;
        if (int rc = d->candidates(images, ns, sigma)) return rc;
        VG_HIP(hipMemcpyAsync(d->h_counts, d->d_counts, sizeof(int) * 4 * d->chunk, hipMemcpyDeviceToHost, d->stream));
        VG_HIP(hipMemcpyAsync(th.data(), d->d_thresh, sizeof(double) * ns, hipMemcpyDeviceToHost, d->stream));
        VG_HIP(hipStreamSynchronize(d->stream));
        for (int s = 0; s < ns; s++) {
            const int nh = d->h_counts[3 * d->chunk + s];
            VG_HIP(hipMemcpy(keys.data(), d->d_hyp + (size_t)s * vg::kSelectMax, sizeof(uint64_t) * nh, hipMemcpyDeviceToHost));
            const int64_t img = c0 + s;
            count[img] = nh;
            val_thresh[img] = th[s];
            n_maxima[img] = d->h_counts[s];
            for (int h = 0; h < std::min(nh, max_out); h++) {
                const int idx = (int)(0xFFFFFFFFu - (uint32_t)(keys[h] & 0xFFFFFFFFu));
                uv[((size_t)img * max_out + h) * 2] = idx % width;
                uv[((size_t)img * max_out + h) * 2 + 1] = idx / width;
            }
        }
    }
    return VG_OK;
}

int vg_corner_detector_stats(const vg_corner_detector *d, double *stats8)
{
    if (!d || !stats8) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    std::copy(d->stats, d->stats + 8, stats8);
    return VG_OK;
}

int vg_corner_detector_chunk(const vg_corner_detector *d, int width, int height, int *chunk)
{
    if (!d || !chunk) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (width < vg::kCornerMinDim || height < vg::kCornerMinDim || width > vg::kCornerMaxDim || height > vg::kCornerMaxDim)
        return fail(VG_ERR_INVALID_ARGUMENT, "image sides must be in [16, 16384]");
    const int tx = (width + vg::kCornerTileW - 1) / vg::kCornerTileW, ty = (height + vg::kCornerTileH - 1) / vg::kCornerTileH;
    const int64_t cp = (int64_t)((width + 1) / 2) * ((height + 1) / 2);
    int c = kCornerMaxChunk;
    while (c > 1 && vg_corner_detector::device_bytes(width, height, c, cp, tx * ty, d->n_corners()) > (size_t)kCornerDeviceBudget) c--;
    *chunk = c;
    return VG_OK;
}

}  // extern "C"
