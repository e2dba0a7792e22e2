// rectify -- the reference's rectification program (test/calibration/rectify.cpp):
//     rectify file.json
// builds the pinhole -> camera maps once (vg_rectify_map) and remaps every listed image through them (vg_remap, same-size
// images batched into one launch), writing img_<k>.pgm into the working directory.
// JSON: camera_params, pinhole_params [width, height, u0, v0, f], xi_eucm_pinhole (any transformFromData form), image_names,
// and optionally "camera_model": "eucm" (the default, as in the reference) | "ucm" | "mei" | "kb" | "ds".
// Images are binary 8-bit PGM (P5) in and out: the project has no image library (the reference reads and writes PNG through
// OpenCV).  Everything is read and checked before the GPU is touched.
// Host-only program on top of the C ABI (include/visgeom_amd.h); links libvisgeom_amd.so and the HIP runtime for the buffers.
#include <string>
#include <vector>

#include "vg_stereo_cli.hpp"

namespace {

using vgcli::die;
using vgcli::Image;
using vgcli::read_pgm;
using vgcli::write_pgm;

constexpr size_t kMaxBatchBytes = size_t(1) << 30;   // source bytes of one vg_remap call

}  // namespace

int main(int argc, char **argv)
{
    vgcli::program() = "rectify";
    if (argc != 2) {
        std::fprintf(stderr, "usage: rectify file.json\n");
        return 2;
    }
    int model = VG_MODEL_EUCM;
    std::vector<double> intr, pinhole;
    double xi[6];
    std::vector<Image> images;
    try {
        const vgjson::Value root = vgjson::parse_file(argv[1]);
        if (root.has("camera_model")) {
            const std::string m = root.at("camera_model").as_string();
            model = m == "eucm" ? VG_MODEL_EUCM : m == "ucm" ? VG_MODEL_UCM : m == "mei" ? VG_MODEL_MEI : m == "kb" ? VG_MODEL_KB : m == "ds" ? VG_MODEL_DS : -1;
            if (model < 0) throw std::runtime_error("unknown camera_model \"" + m + "\"");
        }
        intr = root.at("camera_params").as_vector();
        if ((int)intr.size() != vg_num_intrinsics(model)) throw std::runtime_error("camera_params: wrong number of values for the model");
        pinhole = root.at("pinhole_params").as_vector();
        if (pinhole.size() != 5) throw std::runtime_error("pinhole_params: [width, height, u0, v0, f] expected");
        const std::vector<double> xv = root.at("xi_eucm_pinhole").as_vector();
        if (vg_transform_from_values((int)xv.size(), xv.data(), xi) != VG_OK)
            throw std::runtime_error(std::string("xi_eucm_pinhole: ") + vg_last_error());
        const vgjson::Value &names = root.at("image_names");
        if (names.kind != vgjson::Value::Array) throw std::runtime_error("image_names: an array expected");
        for (const vgjson::Value &n : names.arr) images.push_back(read_pgm(n.as_string()));
    } catch (const std::exception &e) {
        return die(std::string(argv[1]) + ": " + e.what());
    }
    const double pw = pinhole[0], ph = pinhole[1];
    if (!(pw >= 1 && ph >= 1 && pw <= 16384 && ph <= 16384 && pw == (int)pw && ph == (int)ph))
        return die("pinhole_params: width and height must be integers in [1, 16384]");
    const int W = (int)pw, H = (int)ph;
    const size_t map_px = (size_t)W * (size_t)H;

    // the maps, once (rectify.cpp:68)
    float *d_map = nullptr;
    HIPCHECK(hipMalloc(&d_map, 2 * map_px * sizeof(float)));
    VGCHECK(vg_rectify_map(0, nullptr, model, intr.data(), pinhole.data(), xi, d_map, d_map + map_px));

    // runs of consecutive same-size images, one launch each (rectify.cpp:71-78 remaps them one by one)
    std::vector<unsigned char> out;
    unsigned char *d_src = nullptr, *d_dst = nullptr;
    size_t src_cap = 0, dst_cap = 0;
    for (size_t k0 = 0; k0 < images.size();) {
        const int w = images[k0].w, h = images[k0].h;
        const size_t in_px = (size_t)w * (size_t)h;
        size_t k1 = k0 + 1;
        while (k1 < images.size() && images[k1].w == w && images[k1].h == h && (k1 - k0 + 1) * in_px <= kMaxBatchBytes) k1++;
        const size_t n = k1 - k0;
        if (n * in_px > src_cap) {
            if (d_src) HIPCHECK(hipFree(d_src));
            HIPCHECK(hipMalloc(&d_src, n * in_px));
            src_cap = n * in_px;
        }
        if (n * map_px > dst_cap) {
            if (d_dst) HIPCHECK(hipFree(d_dst));
            HIPCHECK(hipMalloc(&d_dst, n * map_px));
            dst_cap = n * map_px;
        }
        for (size_t k = k0; k < k1; k++)
            HIPCHECK(hipMemcpy(d_src + (k - k0) * in_px, images[k].px.data(), in_px, hipMemcpyHostToDevice));
        VGCHECK(vg_remap(0, nullptr, VG_PIXEL_U8, 1, (int64_t)n, w, h, d_src, W, H, d_map, d_map + map_px, 0., d_dst));
        out.resize(n * map_px);
        HIPCHECK(hipMemcpy(out.data(), d_dst, n * map_px, hipMemcpyDeviceToHost));
        for (size_t k = k0; k < k1; k++) {
            try {
                write_pgm("img_" + std::to_string(k) + ".pgm", W, H, out.data() + (k - k0) * map_px);
            } catch (const std::exception &e) {
                return die(e.what());
            }
        }
        k0 = k1;
    }
    if (d_src) HIPCHECK(hipFree(d_src));
    if (d_dst) HIPCHECK(hipFree(d_dst));
    HIPCHECK(hipFree(d_map));
    return 0;
}
