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
#include "vg_stereo_cli.hpp"

using namespace vgcli;

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
        write_pgm(dir + "/inverse_depth.pgm", X, Y, inv.data());
    } catch (const std::exception &e) {
        return die(e.what());
    }
    return 0;
}
