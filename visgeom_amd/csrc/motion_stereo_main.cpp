// motion_stereo -- the reference's depth-from-motion loop (test/reconstruction/stereo_test.cpp:143-172) on files:
//     motion_stereo sequence.json
// reads the keys of the `stereo` program's JSON (camera_params_left / _right, stereo_parameters with its optional
// "motion_stereo_parameters": {"gradient_thresh"}) plus "images": [...] (binary 8-bit PGM, relative to the JSON's directory),
// "transformations": [[6 values], ...] (the pose of each image in the first one's frame, [t, rotvec]; the first image is the key
// frame and its entry is not used) and "sgm_frames" (default 2).  Image i >= 1 goes through EnhancedSgm against the key frame
// while i <= sgm_frames (vg_stereo_*), through MotionStereo::compute with the previous map as the prior after
// (vg_motion_stereo_*).  Writes depth_<i>.pfm and sigma_<i>.pfm next to the JSON.  No filterNoise.
// Everything is read and checked before the GPU is touched.
#include "vg_stereo_cli.hpp"

using namespace vgcli;

int main(int argc, char **argv)
{
    program() = "motion_stereo";
    if (argc != 2) {
        std::fprintf(stderr, "usage: motion_stereo sequence.json\n");
        return 2;
    }
    const std::string dir = dir_of(argv[1]);
    std::vector<double> c1, c2;
    std::vector<double> xi;   // [n][6]
    std::vector<Image> images;
    int sgm_frames = 2;
    vg_motion_stereo_params mp;
    vg_motion_stereo_params_default(&mp);
    vg_stereo_params &p = mp.stereo;
    try {
        const vgjson::Value root = vgjson::parse_file(argv[1]);
        if (root.kind != vgjson::Value::Object) throw std::runtime_error("a JSON object expected");
        c1 = vec6(root, "camera_params_left");
        c2 = vec6(root, "camera_params_right");
        const vgjson::Value &sp = root.at("stereo_parameters");
        read_params(sp, p);
        if (sp.has("motion_stereo_parameters")) {
            const vgjson::Value &m = sp.at("motion_stereo_parameters");
            if (m.kind != vgjson::Value::Object) throw std::runtime_error("motion_stereo_parameters: an object expected");
            if (m.has("gradient_thresh")) mp.gradient_thresh = as_int(m.at("gradient_thresh"), "gradient_thresh");
        }
        if (root.has("sgm_frames")) sgm_frames = as_int(root.at("sgm_frames"), "sgm_frames");
        if (sgm_frames < 0) throw std::runtime_error("sgm_frames must be >= 0");
        const vgjson::Value &im = root.at("images"), &tr = root.at("transformations");
        if (im.kind != vgjson::Value::Array || tr.kind != vgjson::Value::Array) throw std::runtime_error("images, transformations: arrays expected");
        if (im.arr.size() < 2) throw std::runtime_error("images: the key frame and at least one further image expected");
        if (im.arr.size() != tr.arr.size())
            throw std::runtime_error(std::to_string(im.arr.size()) + " images but " + std::to_string(tr.arr.size()) + " transformations");
        xi.resize(6 * im.arr.size());
        for (size_t i = 0; i < im.arr.size(); i++) {
            const std::vector<double> xv = tr.arr[i].as_vector();
            if (vg_transform_from_values((int)xv.size(), xv.data(), &xi[6 * i]) != VG_OK)
                throw std::runtime_error("transformations[" + std::to_string(i) + "]: " + vg_last_error());
        }
        for (size_t i = 0; i < im.arr.size(); i++) {
            images.push_back(read_pgm(resolve(dir, im.arr[i].as_string())));
            const Image &g = images.back();
            if (g.w != p.u_max || g.h != p.v_max)
                throw std::runtime_error("image size " + std::to_string(g.w) + " x " + std::to_string(g.h) + " differs from uMax x vMax = " +
                                         std::to_string(p.u_max) + " x " + std::to_string(p.v_max));
        }
    } catch (const std::exception &e) {
        return die(std::string(argv[1]) + ": " + e.what());
    }

    vg_motion_stereo *m = nullptr;
    VGCHECK(vg_motion_stereo_create(&m, 0, nullptr, c1.data(), c2.data(), &mp));
    int X = 0, Y = 0;
    VGCHECK(vg_motion_stereo_size(m, &X, &Y));
    const size_t img = (size_t)p.u_max * p.v_max, P = (size_t)X * Y;
    unsigned char *d_img = nullptr;
    double *d_out = nullptr;   // depth, sigma, cost
    HIPCHECK(hipMalloc(&d_img, 2 * img));
    HIPCHECK(hipMalloc(&d_out, 3 * P * sizeof(double)));
    HIPCHECK(hipMemcpy(d_img, images[0].px.data(), img, hipMemcpyHostToDevice));
    VGCHECK(vg_motion_stereo_set_base(m, 1, d_img));
    std::vector<double> depth(P), sigma(P);
    bool have_map = false;
    for (size_t i = 1; i < images.size(); i++) {
        HIPCHECK(hipMemcpy(d_img + img, images[i].px.data(), img, hipMemcpyHostToDevice));
        if ((int)i <= sgm_frames) {
            vg_stereo *s = nullptr;
            VGCHECK(vg_stereo_create(&s, 0, nullptr, c1.data(), c2.data(), &xi[6 * i], &p));
            VGCHECK(vg_stereo_compute(s, 1, d_img, d_img + img, d_out, d_out + P, d_out + 2 * P, nullptr));
            vg_stereo_destroy(s);
        } else if (have_map) {
            VGCHECK(vg_motion_stereo_compute(m, 1, &xi[6 * i], d_img + img, d_out, d_out + P, d_out + 2 * P, d_out, d_out + P, d_out + 2 * P, nullptr));
        } else {
            VGCHECK(vg_motion_stereo_compute(m, 1, &xi[6 * i], d_img + img, nullptr, nullptr, nullptr, d_out, d_out + P, d_out + 2 * P, nullptr));
        }
        have_map = true;
        HIPCHECK(hipMemcpy(depth.data(), d_out, P * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(sigma.data(), d_out + P, P * sizeof(double), hipMemcpyDeviceToHost));
        try {
            write_pfm(dir + "/depth_" + std::to_string(i) + ".pfm", X, Y, depth);
            write_pfm(dir + "/sigma_" + std::to_string(i) + ".pfm", X, Y, sigma);
        } catch (const std::exception &e) {
            return die(e.what());
        }
    }
    vg_motion_stereo_destroy(m);
    HIPCHECK(hipFree(d_img));
    HIPCHECK(hipFree(d_out));
    return 0;
}
