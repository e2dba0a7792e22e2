// stereo_accuracy -- the reference's check of its stereo against the renderer's exact depth (test/reconstruction/stereo_test.cpp):
//     stereo_accuracy sequence.json
// reads the keys the reference reads: "trajectory": {"initial", "increment", "step_count"}, "camera_params" (6 EUCM parameters),
// "stereo_parameters" (as the `stereo` and `motion_stereo` programs read it), "render" (the path of a world file as the `render`
// program reads it; its image size must be uMax x vMax), "noise" (an integer >= 0), "sgm" and "filter_noise" (true / false); and
// one key of ours, "cloud_step" (default 9, the reference's constant).
// The key image img1 is rendered at `initial` and its depth buffer is the truth.  Step i in [0, step_count) renders img2 at
// initial o increment^(i + 1); with T = initial^-1 o that pose it runs EnhancedSgm(T) on (img1, img2) while i < 2 or "sgm" is set
// (a fresh vg_stereo handle per step), and MotionStereo::compute(T, img2, carried map) with descriptor_size forced to 7 on the base
// image img1 otherwise; then filterNoise if asked.  A step whose baseline vg_stereo_create refuses ends the program with its error.
// Writes next to the JSON: img_<i>.pgm, depth_<i>.pfm, sigma_<i>.pfm; hist_0_<i+1>.txt, one line per scored pixel in the
// reference's column-major order: truth - depth, truth and sigma as floats; analysis_output.txt, one line per step: the baseline
// |T.trans|, then sqrt(err2 / N) 1000, 100 N / Nmax, dist / Nmax and N / Ngt of vg_depth_compare (sigma_max 10); and at step
// cloud_step cloud.txt, the points of vg_depth_reconstruct with flags 0, one per line as Eigen prints a row vector.
// A nonzero "noise" subtracts, saturating at 0, floor(U noise) from every pixel on the host, U the splitmix64 uniform of
// visgeom_amd/synthetic.py with seed 20260928, stream = image number (0 for img1, i + 1 for step i) and counter = pixel index
// (OpenCV's randu stream cannot be reproduced); the image goes up again.  Everything is read and checked before the GPU is touched.
#include "vg_stereo_cli.hpp"
#include "vg_text_format.hpp"
#include "vg_world_cli.hpp"

using namespace vgcli;

namespace {

constexpr uint64_t kSeed = 20260928ull, kGolden = 0x9E3779B97F4A7C15ull;

uint64_t mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// synthetic.uniform(seed, stream, counter)
double uniform(uint64_t stream, uint64_t counter)
{
    const uint64_t s0 = mix(kSeed * kGolden + mix(stream + 1));
    return (double)(mix(s0 + (counter + 1) * kGolden) >> 11) * (1.0 / 9007199254740992.0);
}

void add_noise(std::vector<unsigned char> &px, int level, uint64_t image)
{
    for (size_t k = 0; k < px.size(); k++) {
        const int v = (int)std::floor(uniform(image, k) * level);
        px[k] = (unsigned char)(px[k] > v ? px[k] - v : 0);
    }
}

bool flag(const vgjson::Value &root, const char *key)
{
    if (root.at(key).kind != vgjson::Value::Bool) throw std::runtime_error(std::string(key) + ": true or false expected");
    return root.at(key).as_bool();
}

void append_g6(std::string &out, double v)
{
    char buf[32];
    if (std::isnan(v)) out += "nan";
    else out.append(buf, (size_t)vgtext::fmt_g6(v, buf));
}

void write_text(const std::string &path, const std::string &text) { write_file(path, std::string(), text.data(), text.size()); }

}  // namespace

int main(int argc, char **argv)
{
    program() = "stereo_accuracy";
    if (argc != 2) {
        std::fprintf(stderr, "usage: stereo_accuracy sequence.json\n");
        return 2;
    }
    const std::string dir = dir_of(argv[1]);
    std::vector<double> cam, xi0, zeta;
    World world;
    int steps = 0, noise = 0, cloud_step = 9;
    bool sgm = false, filter_noise = false;
    vg_motion_stereo_params mp;
    vg_motion_stereo_params_default(&mp);
    vg_stereo_params p;   // of SGM; the motion stereo's copy has descriptor_size 7
    try {
        const vgjson::Value root = vgjson::parse_file(argv[1]);
        if (root.kind != vgjson::Value::Object) throw std::runtime_error("a JSON object expected");
        const vgjson::Value &tr = root.at("trajectory");
        if (tr.kind != vgjson::Value::Object) throw std::runtime_error("trajectory: an object expected");
        xi0 = pose_of(tr.at("initial"), "trajectory.initial");
        zeta = pose_of(tr.at("increment"), "trajectory.increment");
        steps = as_int(tr.at("step_count"), "trajectory.step_count");
        if (steps < 1 || steps > 65535) throw std::runtime_error("trajectory.step_count must be in [1, 65535]");
        cam = vec6(root, "camera_params");
        read_motion_stereo_parameters(root.at("stereo_parameters"), mp);
        p = mp.stereo;
        mp.stereo.desc_length = 7;
        mp.stereo.verbosity = 0;
        noise = as_int(root.at("noise"), "noise");
        if (noise < 0 || noise > 256) throw std::runtime_error("noise must be in [0, 256]");
        sgm = flag(root, "sgm");
        filter_noise = flag(root, "filter_noise");
        if (root.has("cloud_step")) cloud_step = as_int(root.at("cloud_step"), "cloud_step");
        if (cloud_step < 0) throw std::runtime_error("cloud_step must be >= 0");
        read_world(resolve(dir, root.at("render").as_string()), world);
        if (world.width != p.u_max || world.height != p.v_max) throw std::runtime_error("the world's image size differs from uMax x vMax");
    } catch (const std::exception &e) {
        return die(std::string(argv[1]) + ": " + e.what());
    }

    struct Owned {   // released on every way out of main
        vg_render *r = nullptr;
        vg_motion_stereo *m = nullptr;
        vg_depth_fusion *f = nullptr;
        vg_stereo *s = nullptr;
        unsigned char *img = nullptr;
        float *truth = nullptr;
        double *map = nullptr, *cloud = nullptr;
        ~Owned()
        {
            vg_stereo_destroy(s);
            vg_motion_stereo_destroy(m);
            vg_depth_fusion_destroy(f);
            vg_render_destroy(r);
            (void)hipFree(img);
            (void)hipFree(truth);
            (void)hipFree(map);
            (void)hipFree(cloud);
        }
    } d;
    VGCHECK(vg_render_create(&d.r, 0, nullptr, cam.data(), world.width, world.height, (int)world.objects.size(), world.objects.data()));
    VGCHECK(vg_motion_stereo_create(&d.m, 0, nullptr, cam.data(), cam.data(), &mp));
    VGCHECK(vg_depth_fusion_create(&d.f, 0, nullptr, cam.data(), &p));
    int X = 0, Y = 0;
    VGCHECK(vg_depth_fusion_size(d.f, &X, &Y));
    const int W = p.u_max, H = p.v_max;
    const size_t img = (size_t)W * H, P = (size_t)X * Y;
    HIPCHECK(hipMalloc(&d.img, 2 * img));
    HIPCHECK(hipMalloc(&d.truth, img * sizeof(float)));
    HIPCHECK(hipMalloc(&d.map, 3 * P * sizeof(double)));
    unsigned char *img1 = d.img, *img2 = d.img + img;
    double *depth = d.map, *sigma = d.map + P, *cost = d.map + 2 * P;
    std::vector<unsigned char> host(img);
    std::vector<float> truth(img);
    std::vector<double> hd(P), hs(P);

    auto noisy = [&](unsigned char *dev, uint64_t image) -> int {   // the image is left in `host` either way
        HIPCHECK(hipMemcpy(host.data(), dev, img, hipMemcpyDeviceToHost));
        if (noise != 0) {
            add_noise(host, noise, image);
            HIPCHECK(hipMemcpy(dev, host.data(), img, hipMemcpyHostToDevice));
        }
        return 0;
    };
    VGCHECK(vg_render_views(d.r, 1, xi0.data(), img1, d.truth, nullptr, nullptr, nullptr, nullptr));
    HIPCHECK(hipMemcpy(truth.data(), d.truth, img * sizeof(float), hipMemcpyDeviceToHost));
    if (const int rc = noisy(img1, 0)) return rc;
    VGCHECK(vg_motion_stereo_set_base(d.m, 1, img1));

    std::string analysis;
    std::vector<double> xi(6), next(6);
    VGCHECK(vg_mono_odom_compose(xi0.data(), zeta.data(), xi.data()));
    for (int i = 0; i < steps; i++) {
        VGCHECK(vg_render_views(d.r, 1, xi.data(), img2, nullptr, nullptr, nullptr, nullptr, nullptr));
        if (const int rc = noisy(img2, (uint64_t)i + 1)) return rc;
        double T[6];
        VGCHECK(vg_transform_inverse_compose(xi0.data(), xi.data(), T));
        if (i < 2 || sgm) {
            if (vg_stereo_create(&d.s, 0, nullptr, cam.data(), cam.data(), T, &p) != VG_OK)
                return die("step " + std::to_string(i) + ": " + vg_last_error());
            VGCHECK(vg_stereo_compute(d.s, 1, img1, img2, depth, sigma, cost, nullptr));
            vg_stereo_destroy(d.s);
            d.s = nullptr;
        } else {
            VGCHECK(vg_motion_stereo_compute(d.m, 1, T, img2, depth, sigma, cost, depth, sigma, cost, nullptr));
        }
        if (filter_noise) VGCHECK(vg_depth_filter_noise(d.f, 1, depth, sigma, depth, sigma, nullptr));
        std::string cloud_text;
        if (i == cloud_step) {
            int64_t count = 0;
            VGCHECK(vg_depth_reconstruct(d.f, 1, 1, 0, depth, sigma, 0, nullptr, nullptr, nullptr, &count, nullptr));
            std::vector<double> pts((size_t)count * 3);
            if (count > 0) {
                HIPCHECK(hipMalloc(&d.cloud, pts.size() * sizeof(double)));
                vg_recon_outputs out = {};
                out.cloud = d.cloud;
                VGCHECK(vg_depth_reconstruct(d.f, 1, 1, 0, depth, sigma, 0, nullptr, nullptr, nullptr, &count, &out));
                HIPCHECK(hipMemcpy(pts.data(), d.cloud, pts.size() * sizeof(double), hipMemcpyDeviceToHost));
            }
            for (int64_t k = 0; k < count; k++) {
                vgtext::fmt_vec_append(cloud_text, &pts[(size_t)k * 3], 3);
                cloud_text += '\n';
            }
        }
        int64_t counts[3];
        double sums[3];
        VGCHECK(vg_depth_compare(d.f, 1, depth, sigma, d.truth, 10., counts, sums, nullptr));
        HIPCHECK(hipMemcpy(hd.data(), depth, P * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(hs.data(), sigma, P * sizeof(double), hipMemcpyDeviceToHost));
        std::string hist;   // analyzeError's ofs lines: every pixel that Nmax counts
        for (int x = 0; x < X; x++)
            for (int y = 0; y < Y; y++) {
                const float t = truth[(size_t)(y * p.scale + p.v0) * W + (x * p.scale + p.u0)];
                const float dv = (float)hd[(size_t)y * X + x], sv = (float)hs[(size_t)y * X + x];
                if (t == 0.f || dv == 0.f || t != t || dv != dv) continue;
                append_g6(hist, (double)(t - dv));
                hist += "    ";
                append_g6(hist, (double)t);
                hist += "   ";
                append_g6(hist, (double)sv);
                hist += '\n';
            }
        const double ngt = (double)counts[0], nmax = (double)counts[1], n = (double)counts[2];
        append_g6(analysis, std::sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2]));
        const double fig[4] = {std::sqrt(sums[1] / n) * 1000, 100 * n / nmax, sums[2] / nmax, n / ngt};
        for (double v : fig) {
            analysis += "    ";
            append_g6(analysis, v);
        }
        analysis += '\n';
        try {
            const std::string tag = std::to_string(i);
            write_pgm(dir + "/img_" + tag + ".pgm", W, H, host.data());
            write_pfm(dir + "/depth_" + tag + ".pfm", X, Y, hd);
            write_pfm(dir + "/sigma_" + tag + ".pfm", X, Y, hs);
            write_text(dir + "/hist_0_" + std::to_string(i + 1) + ".txt", hist);
            if (i == cloud_step) write_text(dir + "/cloud.txt", cloud_text);
        } catch (const std::exception &e) {
            return die(e.what());
        }
        VGCHECK(vg_mono_odom_compose(xi.data(), zeta.data(), next.data()));
        xi = next;
    }
    try {
        write_text(dir + "/analysis_output.txt", analysis);
    } catch (const std::exception &e) {
        return die(e.what());
    }
    return 0;
}
