// vg_stereo_cli.hpp -- what the `rectify`, `stereo`, `motion_stereo`, `render`, `mono_odom` and `mapping` programs share: binary PGM in
// and out, PFM out, the parameters of ex_epipolar_stereo.json's "stereo_parameters" object with its motion stereo part, path
// handling and the one-line error exit.  Host only.
#pragma once

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

namespace vgcli {

struct Image {
    int w = 0, h = 0;
    std::vector<unsigned char> px;
};

// binary PGM: "P5" <ws> width <ws> height <ws> maxval <one ws> width * height bytes ('#' comments in the header)
inline Image read_pgm(const std::string &path)
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

inline void write_file(const std::string &path, const std::string &header, const void *data, size_t bytes)
{
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    bool ok = std::fwrite(header.data(), 1, header.size(), f) == header.size();
    ok = ok && std::fwrite(data, 1, bytes, f) == bytes;
    if (std::fclose(f) != 0 || !ok) throw std::runtime_error("cannot write " + path);
}

// binary 8-bit PGM
inline void write_pgm(const std::string &path, int w, int h, const unsigned char *px)
{
    write_file(path, "P5\n" + std::to_string(w) + " " + std::to_string(h) + "\n255\n", px, (size_t)w * h);
}

// float32 PFM, little endian (scale -1), rows bottom to top
inline void write_pfm(const std::string &path, int w, int h, const std::vector<double> &v)
{
    std::vector<float> rows((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) rows[(size_t)(h - 1 - y) * w + x] = (float)v[(size_t)y * w + x];
    write_file(path, "Pf\n" + std::to_string(w) + " " + std::to_string(h) + "\n-1.0\n", rows.data(), rows.size() * sizeof(float));
}

inline const char *&program()   // the name die() prints, set first thing in main
{
    static const char *name = "stereo";
    return name;
}

inline int die(const std::string &msg)
{
    std::fprintf(stderr, "%s: %s\n", program(), msg.c_str());
    return 1;
}

#define HIPCHECK(expr)                                                                                  \
    do {                                                                                                \
        const hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return vgcli::die(std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)
#define VGCHECK(expr)                                                                                   \
    do {                                                                                                \
        if ((expr) != VG_OK) return vgcli::die(std::string(#expr) + ": " + vg_last_error());                   \
    } while (0)

inline int as_int(const vgjson::Value &v, const std::string &key)
{
    const double d = v.as_number();
    if (!(d == std::floor(d) && std::fabs(d) < 2e9)) throw std::runtime_error(key + ": an integer expected");
    return (int)d;
}

inline std::vector<double> vec6(const vgjson::Value &root, const char *key)
{
    std::vector<double> v = root.at(key).as_vector();
    if (v.size() != 6) throw std::runtime_error(std::string(key) + ": 6 EUCM parameters expected");
    return v;
}

// SgmParameters(ptree) (eucm_sgm.h:43-55, eucm_stereo.cpp:20-38, scale_parameters.cpp:29-42): unknown keys are ignored
inline void read_params(const vgjson::Value &sp, vg_stereo_params &p)
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

// "stereo_parameters" with its optional "motion_stereo_parameters": {"gradient_thresh"}
inline void read_motion_stereo_parameters(const vgjson::Value &sp, vg_motion_stereo_params &mp)
{
    read_params(sp, mp.stereo);
    if (!sp.has("motion_stereo_parameters")) return;
    const vgjson::Value &m = sp.at("motion_stereo_parameters");
    if (m.kind != vgjson::Value::Object) throw std::runtime_error("motion_stereo_parameters: an object expected");
    if (m.has("gradient_thresh")) mp.gradient_thresh = as_int(m.at("gradient_thresh"), "gradient_thresh");
}

inline std::string dir_of(const std::string &path)
{
    const size_t s = path.find_last_of('/');
    return s == std::string::npos ? std::string(".") : (s == 0 ? std::string("/") : path.substr(0, s));
}

inline std::string resolve(const std::string &dir, const std::string &p) { return !p.empty() && p[0] == '/' ? p : dir + "/" + p; }

}  // namespace vgcli
