// vg_hough_tu.hip -- translation unit of libvisgeom_amd.so: fisheye line detection (section 19 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_hough handle owns the scratch of a chunk of images: the int32 accumulators, the row pass and the blurred accumulators,
// the block counts of the compaction and the compacted maxima with their pinned copy.  A chunk is as many images as fit
// max(1 GiB, one image's scratch); a larger batch is worked through chunk by chunk.  Buffers only grow.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <vector>

#include "vg_handle.hpp"
#include "vg_hough.hpp"
#include "vg_stereo_host.hpp"

struct vg_hough : vgi::HandleBase {
    vgh::Geom g;
    vg_hough_params prm;
    vgh::BlurWeights bw;
    int64_t bins = 0;
    vgi::Counters counters;
    vgi::Grow<int32_t> d_acc;
    vgi::Grow<float> d_rows, d_blur;
    vgi::PackScratch pack;   // counts [image][block], one total per image
    vgi::Grow<vgh::LineRec> d_recs;
    vgi::GrowPinned<vgh::LineRec> h_recs;
};

namespace {

using vgi::fail;
using vgsh::blocks_of;

constexpr int64_t kScratchBudget = int64_t(1) << 30;   // device scratch of one handle, bytes (one image's if that is larger)

// cv::getGaussianKernel(n, sigma, CV_64F) for sigma > 0: exp(-x^2 / (2 sigma^2)) normalised to sum 1, then rounded to float
void gaussian(int n, double sigma, float *w)
{
    double cf[vgh::kMaxBlur];
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

int check_params(const vg_hough_params &p)
{
    if (p.margin < 1) return fail(VG_ERR_INVALID_ARGUMENT, "margin must be at least 1");
    if (p.search_size < 1 || p.search_size > VG_HOUGH_MAX_SEARCH) return fail(VG_ERR_INVALID_ARGUMENT, "search_size must be in [1, 8]");
    if (p.blur_size < VG_HOUGH_MIN_BLUR || p.blur_size > VG_HOUGH_MAX_BLUR || p.blur_size % 2 == 0)
        return fail(VG_ERR_INVALID_ARGUMENT, "blur_size must be odd and in [3, 15]");
    const double v[5] = {p.grad_thresh, p.acc_thresh, p.acc_delta_thresh, p.horizon_ratio, p.blur_sigma};
    if (!vgsh::finite_n(v, 5)) return fail(VG_ERR_INVALID_ARGUMENT, "the thresholds and blur_sigma must be finite");
    if (!(p.blur_sigma > 0.)) return fail(VG_ERR_INVALID_ARGUMENT, "blur_sigma must be positive");
    return VG_OK;
}

int check_call(const vg_hough *s, int64_t n, const void *images)
{
    if (const int rc = vgi::check_items(n, 0, "image")) return rc;
    if (n > 0 && !images) return fail(VG_ERR_INVALID_ARGUMENT, "the images are NULL");
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "hough handle is NULL");
    return VG_OK;
}

// the accumulators of n images, cleared and voted into
int launch_vote(const vg_hough *s, int64_t n, const uint8_t *images, int32_t *acc, unsigned long long *counts)
{
    vgh::VoteArgs a;
    a.g = s->g;
    a.tiles_x = (int)blocks_of(s->g.width, vgh::kTileW);
    a.images = images;
    a.acc = acc;
    a.counts = counts;
    VG_HIP(hipMemsetAsync(acc, 0, (size_t)(n * s->bins) * sizeof(int32_t), s->stream));
    const unsigned tiles = (unsigned)a.tiles_x * blocks_of(s->g.height, vgh::kTileH);
    hipLaunchKernelGGL(vgh::hough_vote_kernel, dim3(tiles, (unsigned)n), dim3(vgh::kLanes), 0, s->stream, a);
    return VG_OK;
}

// the line of one compacted maximum: 16 doubles and the status
void fill_line(const vg_hough *s, const vgh::LineRec &rec, double *L, int32_t *status)
{
    L[0] = rec.u;
    L[1] = rec.v;
    L[2] = rec.val;
    const double nrm = std::sqrt(vgs::dot3(rec.n, rec.n));
    for (int i = 0; i < 3; i++) L[3 + i] = rec.n[i] / nrm;
    const vgs::Poly2 poly = vgh::polynomial(s->g.cam, rec.n);
    const double p6[6] = {poly.kuu, poly.kuv, poly.kvv, poly.ku, poly.kv, poly.k1};
    std::memcpy(L + 6, p6, sizeof p6);
    const bool ok = vgh::end_points(s->g.cam, s->g.width, s->g.height, rec.n, poly, L + 12);
    if (!ok)
        for (int i = 0; i < 4; i++) L[12 + i] = std::numeric_limits<double>::quiet_NaN();
    *status = ok ? VG_HOUGH_OK : VG_HOUGH_NO_END_POINTS;
}

}  // namespace

extern "C" {

void vg_hough_params_default(vg_hough_params *p)
{
    if (!p) return;
    p->margin = 5;
    p->grad_thresh = 0.001;
    p->search_size = 2;
    p->acc_thresh = 7;
    p->acc_delta_thresh = 0.05;
    p->horizon_ratio = 3e-3;
    p->blur_size = 5;
    p->blur_sigma = 0.9;
}

int vg_hough_create(vg_hough **out, int device, void *hip_stream, int width, int height, const double *eucm6, const double *acc_eucm6,
                    const vg_hough_params *params)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (!eucm6 || !acc_eucm6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = vgsh::check_camera(eucm6, "camera")) return rc;
    if (const int rc = vgsh::check_camera(acc_eucm6, "accumulator camera")) return rc;
    vg_hough_params p;
    vg_hough_params_default(&p);
    if (params) p = *params;
    if (const int rc = check_params(p)) return rc;
    const int64_t side_min = 2 * (int64_t)p.margin + 3;
    if (width < side_min || width > VG_HOUGH_MAX_SIDE || height < side_min || height > VG_HOUGH_MAX_SIDE)
        return fail(VG_ERR_INVALID_ARGUMENT, "the image's width and height must be in [2 margin + 3, 16384]");
    const double aw = 2 * acc_eucm6[4], ah = 2 * acc_eucm6[5];   // Mat32f acc(2 v0, 2 u0) (.cpp:369)
    const int acc_min = std::max(2 * p.search_size + 3, (p.blur_size + 1) / 2);
    if (!(aw >= acc_min && aw < VG_HOUGH_MAX_ACC_SIDE + 1 && ah >= acc_min && ah < VG_HOUGH_MAX_ACC_SIDE + 1))
        return fail(VG_ERR_INVALID_ARGUMENT,
                    "the accumulator's sides (int)(2 u0), (int)(2 v0) must be in [2 search_size + 3, 4096] and at least (blur_size + 1) / 2");
    std::unique_ptr<vg_hough> s(new (std::nothrow) vg_hough());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    vgh::Geom &g = s->g;
    for (int i = 0; i < 6; i++) {
        g.cam[i] = eucm6[i];
        g.acc_cam[i] = acc_eucm6[i];
    }
    g.width = width;
    g.height = height;
    g.acc_w = (int)aw;
    g.acc_h = (int)ah;
    g.margin = p.margin;
    g.search_size = p.search_size;
    g.grad_thresh = p.grad_thresh;
    g.acc_thresh = p.acc_thresh;
    g.acc_delta_thresh = p.acc_delta_thresh;
    g.horizon_ratio = p.horizon_ratio;
    s->prm = p;
    s->bins = (int64_t)g.acc_w * g.acc_h;
    s->bw.n = p.blur_size;
    gaussian(p.blur_size, p.blur_sigma, s->bw.w);
    if (const int rc = s->open(device, hip_stream, "line detection")) return rc;
    *out = s.release();
    return VG_OK;
}

void vg_hough_destroy(vg_hough *s) { vgi::destroy(s); }

int vg_hough_size(const vg_hough *s, int *acc_w, int *acc_h)
{
    if (!s || !acc_w || !acc_h) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *acc_w = s->g.acc_w;
    *acc_h = s->g.acc_h;
    return VG_OK;
}

int vg_hough_vote(vg_hough *s, int64_t n, const uint8_t *images, int32_t *acc, int64_t *counts)
{
    if (const int rc = check_call(s, n, images)) return rc;
    if (n > 0 && !acc) return fail(VG_ERR_INVALID_ARGUMENT, "the accumulator is NULL");
    if (n == 0) return VG_OK;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    unsigned long long *dc = nullptr;
    if (const int rc = s->counters.begin(call, n, vgh::kCounts, counts, &dc)) return rc;
    if (const int rc = launch_vote(s, n, images, acc, dc)) return rc;
    VG_HIP(hipGetLastError());
    return s->counters.end(call, n, vgh::kCounts, counts);
}

int vg_hough_detect(vg_hough *s, int64_t n, const uint8_t *images, int max_lines, double *lines, int32_t *status, int32_t *count, float *acc_blur)
{
    if (const int rc = check_call(s, n, images)) return rc;
    if (max_lines < 0 || max_lines > VG_HOUGH_MAX_LINES) return fail(VG_ERR_INVALID_ARGUMENT, "max_lines must be in [0, 65536]");
    if (n > 0 && (!count || (max_lines > 0 && (!lines || !status)))) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n == 0) return VG_OK;
    const int64_t bins = s->bins, nb = blocks_of(bins, vgh::kLanes), img = (int64_t)s->g.width * s->g.height;
    const int64_t per_image = bins * 12 + nb * 8 + (int64_t)max_lines * (int64_t)sizeof(vgh::LineRec);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, kScratchBudget / per_image));
    for (int64_t first = 0; first < n; first += chunk) {
        const int64_t m = std::min(chunk, n - first);
        vgi::Call call(s);
        if (const int rc = call.begin()) return rc;
        if (const int rc = s->d_acc.grow((size_t)(m * bins), "the accumulators")) return rc;
        if (const int rc = s->d_rows.grow((size_t)(m * bins), "the blur's row pass")) return rc;
        if (!acc_blur)
            if (const int rc = s->d_blur.grow((size_t)(m * bins), "the blurred accumulators")) return rc;
        if (const int rc = s->pack.grow((size_t)(m * nb), (size_t)m, "the maxima's block counts")) return rc;
        if (const int rc = s->d_recs.grow((size_t)(m * std::max(max_lines, 1)), "the maxima")) return rc;
        if (const int rc = s->h_recs.grow((size_t)(m * std::max(max_lines, 1)), "the maxima's staging")) return rc;
        float *blur = acc_blur ? acc_blur + first * bins : s->d_blur.get();
        if (const int rc = launch_vote(s, m, images + first * img, s->d_acc, nullptr)) return rc;
        const dim3 grid((unsigned)nb, (unsigned)m), block(vgh::kLanes);
        hipLaunchKernelGGL((vgh::hough_blur_kernel<false, int32_t>), grid, block, 0, s->stream, (const int32_t *)s->d_acc.get(), s->d_rows.get(),
                           s->g.acc_w, s->g.acc_h, s->bw);
        hipLaunchKernelGGL((vgh::hough_blur_kernel<true, float>), grid, block, 0, s->stream, (const float *)s->d_rows.get(), blur, s->g.acc_w,
                           s->g.acc_h, s->bw);
        vgh::MaximaArgs a;
        a.g = s->g;
        a.blur = blur;
        a.block_counts = s->pack.counts;
        a.block_offsets = s->pack.offsets;
        a.max_lines = max_lines;
        a.recs = s->d_recs;
        hipLaunchKernelGGL((vgh::hough_maxima_kernel<false>), grid, block, 0, s->stream, a);
        hipLaunchKernelGGL(vgc::scan_block_counts_items_kernel<vgh::kLanes>, dim3((unsigned)m), block, 0, s->stream,
                           (const unsigned *)s->pack.counts.get(), s->pack.offsets.get(), (int)nb, s->pack.totals.get());
        if (max_lines > 0) hipLaunchKernelGGL((vgh::hough_maxima_kernel<true>), grid, block, 0, s->stream, a);
        VG_HIP(hipGetLastError());
        if (const int rc = s->pack.fetch(s->stream, (size_t)m)) return rc;
        // every slot is copied; the host reads the written ones only
        if (max_lines > 0)
            VG_HIP(hipMemcpyAsync(s->h_recs, s->d_recs, (size_t)(m * max_lines) * sizeof(vgh::LineRec), hipMemcpyDeviceToHost, s->stream));
        if (const int rc = call.finish()) return rc;
        for (int64_t k = 0; k < m; k++) {
            const int64_t total = s->pack.h_totals.get()[k], item = first + k;
            count[item] = (int32_t)total;
            for (int64_t j = 0; j < std::min<int64_t>(total, max_lines); j++)
                fill_line(s, s->h_recs.get()[k * max_lines + j], lines + (item * max_lines + j) * VG_HOUGH_LINE, status + item * max_lines + j);
        }
    }
    return VG_OK;
}

int vg_hough_polynomial(const double *eucm6, const double *plane3, double *poly6)
{
    if (!eucm6 || !plane3 || !poly6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    const vgs::Poly2 s = vgh::polynomial(eucm6, plane3);
    const double p6[6] = {s.kuu, s.kuv, s.kvv, s.ku, s.kv, s.k1};
    std::memcpy(poly6, p6, sizeof p6);
    return VG_OK;
}

int vg_hough_end_points(int width, int height, const double *eucm6, const double *plane3, const double *poly6, double *pt4, int *status)
{
    if (!eucm6 || !plane3 || !poly6 || !pt4 || !status) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (width < 1 || width > VG_HOUGH_MAX_SIDE || height < 1 || height > VG_HOUGH_MAX_SIDE)
        return fail(VG_ERR_INVALID_ARGUMENT, "the image's width and height must be in [1, 16384]");
    const vgs::Poly2 poly = {poly6[0], poly6[1], poly6[2], poly6[3], poly6[4], poly6[5]};
    const bool ok = vgh::end_points(eucm6, width, height, plane3, poly, pt4);
    if (!ok)
        for (int i = 0; i < 4; i++) pt4[i] = std::numeric_limits<double>::quiet_NaN();
    *status = ok ? VG_HOUGH_OK : VG_HOUGH_NO_END_POINTS;
    return VG_OK;
}

int vg_hough_trace(const double *poly6, const double *pt4, int max_steps, int32_t *uv, int *n)
{
    if (!poly6 || !pt4 || !n || (max_steps > 0 && !uv)) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (max_steps < 0 || max_steps > VG_HOUGH_MAX_TRACE) return fail(VG_ERR_INVALID_ARGUMENT, "max_steps must be in [0, 1500]");
    for (int i = 0; i < 4; i++)
        if (!(std::fabs(pt4[i]) <= (double)(1 << 24))) return fail(VG_ERR_INVALID_ARGUMENT, "the end points must be within +-2^24");
    const vgs::Poly2 poly = {poly6[0], poly6[1], poly6[2], poly6[3], poly6[4], poly6[5]};
    *n = vgh::trace(poly, pt4, max_steps, uv);
    return VG_OK;
}

}  // extern "C"
