// stereo -- the reference's dense stereo example (test/reconstruction/stereo_single_pair.cpp):
//     stereo file.json
// reads ex_epipolar_stereo.json's schema (camera_params_left / _right, stereo_transformation, image_left / _right, brightness,
// stereo_parameters { scale keys, stereo_parameters {...}, sgm_stereo_parameters {...} }), runs EnhancedSgm::computeStereo on
// the GPU (vg_stereo_create / vg_stereo_compute) and writes, next to the JSON file: depth.pfm and sigma.pfm (float32 PFM, rows
// bottom to top as the format stores them) and inverse_depth.pgm (toInverseMat x brightness / 100 x 255, rounded, saturated)
// where the reference calls imshow.  Relative image paths are resolved against the JSON file's directory.
// Images are binary 8-bit PGM (P5): the project has no image library.  Everything is read and checked
// before the GPU is touched.
// Host-only program on top of the C ABI (include/visgeom_amd.h); links libvisgeom_amd.so and the HIP runtime for the buffers.
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/visgeom_amd.h"
#include "vg_json.hpp"

namespace {

struct Image {
    int w = 0, h = 0;
    std::vector<unsigned char> px;
};

// binary PGM: "P5" <ws> width <ws> height <ws> maxval <one ws> width * height bytes ('#' comments in the header)
Image read_pgm(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::string data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t pos = 0;
    auto skip_ws = [&]() {
        while (pos < data.size()) {
            if (data[pos] == '#') {
                while (pos < data.size() && data[pos] != '\n') pos++;
            } else if (std::isspace((unsigned char)data[pos])) {
                pos++;
            } else {
                break;
            }
        }
    };
    auto number = [&]() {
        skip_ws();
        long long v = 0;
        size_t digits = 0;
        while (pos < data.size() && std::isdigit((unsigned char)data[pos]) && digits < 12) v = v * 10 + (data[pos++] - '0'), digits++;
        if (!digits || (pos < data.size() && std::isdigit((unsigned char)data[pos]))) throw std::runtime_error(path + ": malformed PGM header");
        return v;
    };
    if (data.size() < 2 || data[0] != 'P' || data[1] != '5') throw std::runtime_error(path + ": not a binary PGM (P5)");
    pos = 2;
    const long long w = number(), h = number(), maxval = number();
    if (w < 1 || h < 1 || w > 16384 || h > 16384) throw std::runtime_error(path + ": image size out of range");
    if (maxval < 1 || maxval > 255) throw std::runtime_error(path + ": only 8-bit PGM is supported");
    if (pos >= data.size() || !std::isspace((unsigned char)data[pos])) throw std::runtime_error(path + ": malformed PGM header");
    pos++;
    if (data.size() - pos < (size_t)(w * h)) throw std::runtime_error(path + ": truncated PGM");
    Image im;
    im.w = (int)w;
    im.h = (int)h;
    im.px.assign(data.begin() + (std::ptrdiff_t)pos, data.begin() + (std::ptrdiff_t)(pos + (size_t)(w * h)));
    return im;
}

void write_file(const std::string &path, const std::string &header, const void *data, size_t bytes)
{
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    bool ok = std::fwrite(header.data(), 1, header.size(), f) == header.size();
    ok = ok && std::fwrite(data, 1, bytes, f) == bytes;
    if (std::fclose(f) != 0 || !ok) throw std::runtime_error("cannot write " + path);
}

// float32 PFM, little endian (scale -1), rows bottom to top
void write_pfm(const std::string &path, int w, int h, const std::vector<double> &v)
{
    std::vector<float> rows((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) rows[(size_t)(h - 1 - y) * w + x] = (float)v[(size_t)y * w + x];
    write_file(path, "Pf\n" + std::to_string(w) + " " + std::to_string(h) + "\n-1.0\n", rows.data(), rows.size() * sizeof(float));
}

int die(const std::string &msg)
{
    std::fprintf(stderr, "stereo: %s\n", msg.c_str());
    return 1;
}

#define HIPCHECK(expr)                                                                                  \
    do {                                                                                                \
        const hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return die(std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)
#define VGCHECK(expr)                                                                                   \
    do {                                                                                                \
        if ((expr) != VG_OK) return die(std::string(#expr) + ": " + vg_last_error());                   \
    } while (0)

int as_int(const vgjson::Value &v, const std::string &key)
{
    const double d = v.as_number();
    if (!(d == std::floor(d) && std::fabs(d) < 2e9)) throw std::runtime_error(key + ": an integer expected");
    return (int)d;
}

std::vector<double> vec6(const vgjson::Value &root, const char *key)
{
    std::vector<double> v = root.at(key).as_vector();
    if (v.size() != 6) throw std::runtime_error(std::string(key) + ": 6 EUCM parameters expected");
    return v;
}

// SgmParameters(ptree) (eucm_sgm.h:43-55, eucm_stereo.cpp:20-38, scale_parameters.cpp:29-42): unknown keys are ignored
void read_params(const vgjson::Value &sp, vg_stereo_params &p)
{
    if (sp.kind != vgjson::Value::Object) throw std::runtime_error("stereo_parameters: an object expected");
    for (const auto &kv : sp.obj) {
        const std::string &k = kv.first;
        const vgjson::Value &v = kv.second;
        if (k == "scale") p.scale = as_int(v, k);
        else if (k == "u0") p.u0 = as_int(v, k);
        else if (k == "v0") p.v0 = as_int(v, k);
        else if (k == "uMax") p.u_max = as_int(v, k);
        else if (k == "vMax") p.v_max = as_int(v, k);
        else if (k == "xMax") p.x_max = as_int(v, k);
        else if (k == "yMax") p.y_max = as_int(v, k);
        else if (k == "equal_margins" && v.as_bool()) p.equal_margins = 1;
    }
    if (sp.has("stereo_parameters")) {
        const vgjson::Value &s = sp.at("stereo_parameters");
        if (s.kind != vgjson::Value::Object) throw std::runtime_error("stereo_parameters.stereo_parameters: an object expected");
        for (const auto &kv : s.obj) {
            const std::string &k = kv.first;
            const vgjson::Value &v = kv.second;
            if (k == "disparity_max") p.disp_max = as_int(v, k);
            else if (k == "error_max") p.error_max = as_int(v, k);
            else if (k == "verbosity") p.verbosity = as_int(v, k);
            else if (k == "hypotheses") p.hypotheses = as_int(v, k);
            else if (k == "hypo_difference") p.hypo_difference = as_int(v, k);
            else if (k == "flaw_cost") p.flaw_cost = as_int(v, k);
            else if (k == "descriptor_size") p.desc_length = as_int(v, k);
            else if (k == "descriptor_response_thresh") p.desc_resp_thresh = as_int(v, k);
            else if (k == "num_epipolar_planes") p.num_epipolar_planes = as_int(v, k);
            else if (k == "epipole_margin") {
                const int m = as_int(v, k);
                if (std::abs(m) > 46340) throw std::runtime_error("epipole_margin out of range");
                p.epipole_margin = m * m;
            } else if (k == "scales") {
                if (v.kind != vgjson::Value::Array || v.arr.empty() || v.arr.size() > 8)
                    throw std::runtime_error("scales: an array of 1 to 8 integers expected");
                p.n_scales = (int)v.arr.size();
                for (int i = 0; i < 8; i++) p.scales[i] = i < p.n_scales ? as_int(v.arr[i], k) : 0;
            }
        }
    }
    if (sp.has("sgm_stereo_parameters")) {
        const vgjson::Value &s = sp.at("sgm_stereo_parameters");
        if (s.kind != vgjson::Value::Object) throw std::runtime_error("sgm_stereo_parameters: an object expected");
        for (const auto &kv : s.obj) {
            const std::string &k = kv.first;
            const vgjson::Value &v = kv.second;
            if (k == "step_cost") p.step_cost = as_int(v, k);
            else if (k == "jump_cost") p.jump_cost = as_int(v, k);
            else if (k == "image_based_cost") p.image_based_cost = v.as_bool() ? 1 : 0;
            else if (k == "salient_points_only") p.salient_points_only = v.as_bool() ? 1 : 0;
            else if (k == "use_uv_cache") p.use_uv_cache = v.as_bool() ? 1 : 0;
        }
    }
    if (p.hypotheses != 1) throw std::runtime_error("hypotheses must be 1 (multi-hypothesis SGM is not provided)");
}

std::string dir_of(const std::string &path)
{
    const size_t s = path.find_last_of('/');
    return s == std::string::npos ? std::string(".") : (s == 0 ? std::string("/") : path.substr(0, s));
}

std::string resolve(const std::string &dir, const std::string &p) { return !p.empty() && p[0] == '/' ? p : dir + "/" + p; }

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: stereo file.json\n");
        return 2;
    }
    const std::string dir = dir_of(argv[1]);
    std::vector<double> c1, c2;
    double xi[6];
    int brightness = 0;
    vg_stereo_params p;
    vg_stereo_params_default(&p);
    Image im1, im2;
    try {
        const vgjson::Value root = vgjson::parse_file(argv[1]);
        if (root.kind != vgjson::Value::Object) throw std::runtime_error("a JSON object expected");
        c1 = vec6(root, "camera_params_left");
        c2 = vec6(root, "camera_params_right");
        const std::vector<double> xv = root.at("stereo_transformation").as_vector();
        if (vg_transform_from_values((int)xv.size(), xv.data(), xi) != VG_OK)
            throw std::runtime_error(std::string("stereo_transformation: ") + vg_last_error());
        brightness = as_int(root.at("brightness"), "brightness");
        read_params(root.at("stereo_parameters"), p);
        im1 = read_pgm(resolve(dir, root.at("image_left").as_string()));
        im2 = read_pgm(resolve(dir, root.at("image_right").as_string()));
        for (const Image *im : {&im1, &im2})
            if (im->w != p.u_max || im->h != p.v_max)
                throw std::runtime_error("image size " + std::to_string(im->w) + " x " + std::to_string(im->h) + " differs from uMax x vMax = " +
                                         std::to_string(p.u_max) + " x " + std::to_string(p.v_max));
    } catch (const std::exception &e) {
        return die(std::string(argv[1]) + ": " + e.what());
    }

    vg_stereo *s = nullptr;
    VGCHECK(vg_stereo_create(&s, 0, nullptr, c1.data(), c2.data(), xi, &p));
    int X = 0, Y = 0;
    VGCHECK(vg_stereo_size(s, &X, &Y));
    const size_t img = (size_t)p.u_max * p.v_max, P = (size_t)X * Y;
    unsigned char *d_img = nullptr;
    double *d_out = nullptr;
    HIPCHECK(hipMalloc(&d_img, 2 * img));
    HIPCHECK(hipMalloc(&d_out, 2 * P * sizeof(double)));
    HIPCHECK(hipMemcpy(d_img, im1.px.data(), img, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_img + img, im2.px.data(), img, hipMemcpyHostToDevice));
    VGCHECK(vg_stereo_compute(s, 1, d_img, d_img + img, d_out, d_out + P, nullptr, nullptr));
    std::vector<double> depth(P), sigma(P);
    HIPCHECK(hipMemcpy(depth.data(), d_out, P * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(sigma.data(), d_out + P, P * sizeof(double), hipMemcpyDeviceToHost));
    vg_stereo_destroy(s);
    HIPCHECK(hipFree(d_img));
    HIPCHECK(hipFree(d_out));

    // DepthMap::toInverseMat (depth_map.cpp:649-661) times brightness / 100, shown by imshow as x 255
    std::vector<unsigned char> inv(P);
    for (size_t i = 0; i < P; i++) {
        const float f = depth[i] < 1e-3 ? 0.f : (float)(1 / depth[i]);
        const float scaled = (float)((double)f * (brightness / 100.));
        const double v = std::nearbyint((double)scaled * 255.);
        inv[i] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
    try {
        write_pfm(dir + "/depth.pfm", X, Y, depth);
        write_pfm(dir + "/sigma.pfm", X, Y, sigma);
        write_file(dir + "/inverse_depth.pgm", "P5\n" + std::to_string(X) + " " + std::to_string(Y) + "\n255\n", inv.data(), inv.size());
    } catch (const std::exception &e) {
        return die(e.what());
    }
    return 0;
}
