// motion_stereo -- the reference's depth-from-motion loop (test/reconstruction/stereo_test.cpp:143-172) on files:
//     motion_stereo sequence.json
// reads the keys of the `stereo` program's JSON (camera_params_left / _right, stereo_parameters with its optional
// "motion_stereo_parameters": {"gradient_thresh"}) plus "images": [...] (binary 8-bit PGM, relative to the JSON's directory),
// "transformations": [[6 values], ...] (the pose of each image in the first one's frame, [t, rotvec]; the first image is the key
// frame and its entry is not used) and "sgm_frames" (default 2).  Image i >= 1 goes through EnhancedSgm against the key frame
// while i <= sgm_frames (vg_stereo_*), through MotionStereo::compute with the previous map as the prior after
// (vg_motion_stereo_*).  Writes depth_<i>.pfm and sigma_<i>.pfm next to the JSON.
// Two optional keys (vg_depth_*, section 11 of the C ABI); a file without them runs as it always did:
//   "filter_noise": true      DepthMap::filterNoise on the map of every such frame before it is written and carried on, as
//                             improveStereo does (src/localization/mapping.cpp:186-187)
//   "key_frames": [i, ...]    strictly increasing, each in [1, images - 1], both cameras equal.  At image i the program does
//                             pushInterFrame (mapping.cpp:199-220) instead: with `base` the pose of image i in the current key
//                             frame, SGM with image i as camera 1 and the key image as camera 2 under base^-1, filterNoise of
//                             that map (always), the carried map warped by `base`, the SGM map merged into it; image i becomes
//                             the key frame and later poses are re-expressed in its frame.  Without a carried map only the SGM
//                             map is kept (MAP_INIT).  depth_<i>.pfm / sigma_<i>.pfm hold the map in the new key frame.
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
    bool filter_noise = false;
    std::vector<char> is_key;      // [images]: image i becomes the key frame
    std::vector<double> rel, inv;  // [images][6]: the pose of image i in the key frame current at i, and its inverse at a key frame
    vg_motion_stereo_params mp;
    vg_motion_stereo_params_default(&mp);
    vg_stereo_params &p = mp.stereo;
    try {
        const vgjson::Value root = vgjson::parse_file(argv[1]);
        if (root.kind != vgjson::Value::Object) throw std::runtime_error("a JSON object expected");
        c1 = vec6(root, "camera_params_left");
        c2 = vec6(root, "camera_params_right");
        read_motion_stereo_parameters(root.at("stereo_parameters"), mp);
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
        if (root.has("filter_noise")) {
            if (root.at("filter_noise").kind != vgjson::Value::Bool) throw std::runtime_error("filter_noise: true or false expected");
            filter_noise = root.at("filter_noise").as_bool();
        }
        is_key.assign(images.size(), 0);
        if (root.has("key_frames")) {
            const vgjson::Value &kf = root.at("key_frames");
            if (kf.kind != vgjson::Value::Array) throw std::runtime_error("key_frames: an array of image indices expected");
            if (!kf.arr.empty() && c1 != c2)
                throw std::runtime_error("key_frames: camera_params_left and camera_params_right must be equal (a key frame is taken by the second camera)");
            int last = 0;
            for (const vgjson::Value &v : kf.arr) {
                const int i = as_int(v, "key_frames");
                if (i < 1 || i > (int)images.size() - 1)
                    throw std::runtime_error("key_frames: index " + std::to_string(i) + " is not in [1, " + std::to_string(images.size() - 1) + "]");
                if (i <= last) throw std::runtime_error("key_frames: the indices must be strictly increasing");
                is_key[(size_t)i] = 1;
                last = i;
            }
        }
        rel = xi;
        inv.assign(xi.size(), 0.);
        for (size_t i = 1, key = 0; i < images.size(); i++) {
            if (key > 0 && vg_transform_inverse_compose(&xi[6 * key], &xi[6 * i], &rel[6 * i]) != VG_OK) throw std::runtime_error(vg_last_error());
            if (is_key[i]) {
                if (vg_transform_inverse(&rel[6 * i], &inv[6 * i]) != VG_OK) throw std::runtime_error(vg_last_error());
                key = i;
            }
        }
    } catch (const std::exception &e) {
        return die(std::string(argv[1]) + ": " + e.what());
    }

    bool any_key = false;
    for (char k : is_key) any_key = any_key || k;
    vg_motion_stereo *m = nullptr;
    VGCHECK(vg_motion_stereo_create(&m, 0, nullptr, c1.data(), c2.data(), &mp));
    int X = 0, Y = 0;
    VGCHECK(vg_motion_stereo_size(m, &X, &Y));
    vg_depth_fusion *fusion = nullptr;
    if (filter_noise || any_key) VGCHECK(vg_depth_fusion_create(&fusion, 0, nullptr, c1.data(), &p));
    const size_t img = (size_t)p.u_max * p.v_max, P = (size_t)X * Y;
    unsigned char *d_img = nullptr;
    double *d_out = nullptr;   // depth, sigma, cost; with key frames two more triples: the SGM map and the warped map
    HIPCHECK(hipMalloc(&d_img, 2 * img));
    HIPCHECK(hipMalloc(&d_out, (any_key ? 9 : 3) * P * sizeof(double)));
    double *d_sgm = d_out + 3 * P, *d_warp = d_out + 6 * P;
    HIPCHECK(hipMemcpy(d_img, images[0].px.data(), img, hipMemcpyHostToDevice));
    VGCHECK(vg_motion_stereo_set_base(m, 1, d_img));
    std::vector<double> depth(P), sigma(P);
    bool have_map = false;
    for (size_t i = 1; i < images.size(); i++) {
        HIPCHECK(hipMemcpy(d_img + img, images[i].px.data(), img, hipMemcpyHostToDevice));
        const double *pose = &rel[6 * i];
        if (is_key[i]) {   // pushInterFrame
            vg_stereo *s = nullptr;
            double *d_new = have_map ? d_sgm : d_out;
            VGCHECK(vg_stereo_create(&s, 0, nullptr, c1.data(), c2.data(), &inv[6 * i], &p));
            VGCHECK(vg_stereo_compute(s, 1, d_img + img, d_img, d_new, d_new + P, d_new + 2 * P, nullptr));
            vg_stereo_destroy(s);
            VGCHECK(vg_depth_filter_noise(fusion, 1, d_new, d_new + P, d_new, d_new + P, nullptr));
            if (have_map) {
                VGCHECK(vg_depth_warp(fusion, 1, pose, d_out, d_out + P, d_out + 2 * P, d_warp, d_warp + P, d_warp + 2 * P, nullptr));
                VGCHECK(vg_depth_merge(fusion, 1, d_warp, d_warp + P, d_sgm, d_sgm + P, nullptr));
                HIPCHECK(hipMemcpy(d_out, d_warp, 3 * P * sizeof(double), hipMemcpyDeviceToDevice));
            }
            HIPCHECK(hipMemcpy(d_img, d_img + img, img, hipMemcpyDeviceToDevice));
            VGCHECK(vg_motion_stereo_set_base(m, 1, d_img));
        } else {
            if ((int)i <= sgm_frames) {
                vg_stereo *s = nullptr;
                VGCHECK(vg_stereo_create(&s, 0, nullptr, c1.data(), c2.data(), pose, &p));
                VGCHECK(vg_stereo_compute(s, 1, d_img, d_img + img, d_out, d_out + P, d_out + 2 * P, nullptr));
                vg_stereo_destroy(s);
            } else if (have_map) {
                VGCHECK(vg_motion_stereo_compute(m, 1, pose, d_img + img, d_out, d_out + P, d_out + 2 * P, d_out, d_out + P, d_out + 2 * P, nullptr));
            } else {
                VGCHECK(vg_motion_stereo_compute(m, 1, pose, d_img + img, nullptr, nullptr, nullptr, d_out, d_out + P, d_out + 2 * P, nullptr));
            }
            if (filter_noise) VGCHECK(vg_depth_filter_noise(fusion, 1, d_out, d_out + P, d_out, d_out + P, nullptr));
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
    vg_depth_fusion_destroy(fusion);
    HIPCHECK(hipFree(d_img));
    HIPCHECK(hipFree(d_out));
    return 0;
}
