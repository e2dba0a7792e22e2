// mono_odom -- the reference's monocular odometry loop (test/localization/mono_odom_test.cpp) on files:
//     mono_odom sequence.json
// reads what MonoOdometry(ptree) reads -- "xi_base_camera" (a transform literal), "camera_params" (6 EUCM parameters) and
// "stereo_parameters" (as the `stereo` and `motion_stereo` programs read it) -- and one of two inputs:
//   the reference's   "render": the path of a world file as the `render` program reads it (its "views" are not used; its image
//                     size must be uMax x vMax) and "trajectory": {"initial", "increment", "step_count"}: frame i is rendered at
//                     xi_i o xi_base_camera, xi_0 = initial, xi_(i+1) = xi_i o increment, on the device, and xi_i is fed as the
//                     wheel odometry
//   ours              "images": [...] (binary 8-bit PGM, relative to the JSON's directory) and "odometry": [pose, ...], one per image
// Optional keys of ours: "mono_odom_parameters": {"min_init_dist", "max_dist", "max_angle", "min_scale_length", "max_scale_ratio",
// "num_scales"} and "warp": true.  Writes next to the JSON: trajectory.txt, one line per frame -- the index, the state after the
// frame, the action, the composed pose xi_global o xi_local as six numbers and K, the numbers as the reference prints them;
// depth_<k>.pfm / sigma_<k>.pfm, the map in key frame k when it was made, and depth_final.pfm / sigma_final.pfm at the end;
// with "warp", warp_<i>.pgm for every frame with a map: image i seen from the key frame through the map and the frame's pose.
// Everything is read and checked before the GPU is touched.
#include "vg_stereo_cli.hpp"
#include "vg_text_format.hpp"
#include "vg_world_cli.hpp"

using namespace vgcli;

namespace {

const char *const kStates[] = {"BEGIN", "SPARSE_INIT", "READY"};
const char *const kActions[] = {"FIRST", "WAITING", "SPARSE_INIT_KEYFRAME", "REFINED", "KEYFRAME", "DISCARDED"};

}  // namespace

int main(int argc, char **argv)
{
    program() = "mono_odom";
    if (argc != 2) {
        std::fprintf(stderr, "usage: mono_odom sequence.json\n");
        return 2;
    }
    const std::string dir = dir_of(argv[1]);
    std::vector<double> cam, xbc, odometry;   // odometry: [frames][6]
    std::vector<Image> images;                // our mode
    World world;                              // the reference's mode
    bool rendered = false, warp = false;
    vg_mono_odom_params mp;
    vg_mono_odom_params_default(&mp);
    vg_stereo_params &p = mp.motion.stereo;
    try {
        const vgjson::Value root = vgjson::parse_file(argv[1]);
        if (root.kind != vgjson::Value::Object) throw std::runtime_error("a JSON object expected");
        cam = vec6(root, "camera_params");
        xbc = pose_of(root.at("xi_base_camera"), "xi_base_camera");
        read_motion_stereo_parameters(root.at("stereo_parameters"), mp.motion);
        if (root.has("mono_odom_parameters")) {
            const vgjson::Value &m = root.at("mono_odom_parameters");
            if (m.kind != vgjson::Value::Object) throw std::runtime_error("mono_odom_parameters: an object expected");
            for (const auto &kv : m.obj) {
                const std::string &k = kv.first;
                if (k == "min_init_dist") mp.min_init_dist = kv.second.as_number();
                else if (k == "max_dist") mp.max_dist = kv.second.as_number();
                else if (k == "max_angle") mp.max_angle = kv.second.as_number();
                else if (k == "min_scale_length") mp.min_scale_length = kv.second.as_number();
                else if (k == "max_scale_ratio") mp.max_scale_ratio = kv.second.as_number();
                else if (k == "num_scales") mp.num_scales = as_int(kv.second, k);
                else throw std::runtime_error("mono_odom_parameters: unknown key " + k);
            }
        }
        if (root.has("warp")) {
            if (root.at("warp").kind != vgjson::Value::Bool) throw std::runtime_error("warp: true or false expected");
            warp = root.at("warp").as_bool();
        }
        rendered = root.has("render");
        if (rendered == root.has("images")) throw std::runtime_error("exactly one of \"render\" and \"images\" expected");
        if (rendered) {
            read_world(resolve(dir, root.at("render").as_string()), world);
            if (world.width != p.u_max || world.height != p.v_max) throw std::runtime_error("the world's image size differs from uMax x vMax");
            const vgjson::Value &tr = root.at("trajectory");
            if (tr.kind != vgjson::Value::Object) throw std::runtime_error("trajectory: an object expected");
            std::vector<double> xi = pose_of(tr.at("initial"), "trajectory.initial");
            const std::vector<double> zeta = pose_of(tr.at("increment"), "trajectory.increment");
            const int steps = as_int(tr.at("step_count"), "trajectory.step_count");
            if (steps < 1 || steps > 65535) throw std::runtime_error("trajectory.step_count must be in [1, 65535]");
            for (int i = 0; i < steps; i++) {
                odometry.insert(odometry.end(), xi.begin(), xi.end());
                std::vector<double> next(6);
                if (vg_mono_odom_compose(xi.data(), zeta.data(), next.data()) != VG_OK) throw std::runtime_error(vg_last_error());
                xi = next;
            }
        } else {
            const vgjson::Value &im = root.at("images"), &od = root.at("odometry");
            if (im.kind != vgjson::Value::Array || od.kind != vgjson::Value::Array) throw std::runtime_error("images, odometry: arrays expected");
            if (im.arr.empty() || im.arr.size() != od.arr.size()) throw std::runtime_error("one odometry pose per image and at least one image expected");
            for (size_t i = 0; i < im.arr.size(); i++) {
                const std::vector<double> xi = pose_of(od.arr[i], "odometry[" + std::to_string(i) + "]");
                odometry.insert(odometry.end(), xi.begin(), xi.end());
                images.push_back(read_pgm(resolve(dir, im.arr[i].as_string())));
                if (images.back().w != p.u_max || images.back().h != p.v_max) throw std::runtime_error("an image's size differs from uMax x vMax");
            }
        }
    } catch (const std::exception &e) {
        return die(std::string(argv[1]) + ": " + e.what());
    }

    struct Owned {   // released on every way out of main
        vg_mono_odom *m = nullptr;
        vg_render *r = nullptr;
        unsigned char *img = nullptr, *warped = nullptr;
        ~Owned()
        {
            vg_mono_odom_destroy(m);
            vg_render_destroy(r);
            (void)hipFree(img);
            (void)hipFree(warped);
        }
    } d;
    VGCHECK(vg_mono_odom_create(&d.m, 0, nullptr, cam.data(), xbc.data(), p.u_max, p.v_max, &mp));
    if (rendered) VGCHECK(vg_render_create(&d.r, 0, nullptr, cam.data(), world.width, world.height, (int)world.objects.size(), world.objects.data()));
    int W = 0, H = 0, X = 0, Y = 0;
    VGCHECK(vg_mono_odom_size(d.m, &W, &H, &X, &Y));
    const size_t img = (size_t)W * H, P = (size_t)X * Y, frames = odometry.size() / 6;
    HIPCHECK(hipMalloc(&d.img, img));
    HIPCHECK(hipMalloc(&d.warped, img));
    std::vector<double> depth(P), sigma(P);
    std::vector<unsigned char> host(img);
    std::string trajectory;
    auto write_map = [&](const std::string &tag) -> int {
        const double *dd = nullptr, *ds = nullptr, *dc = nullptr;
        VGCHECK(vg_mono_odom_map(d.m, &dd, &ds, &dc));
        HIPCHECK(hipMemcpy(depth.data(), dd, P * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(sigma.data(), ds, P * sizeof(double), hipMemcpyDeviceToHost));
        try {
            write_pfm(dir + "/depth_" + tag + ".pfm", X, Y, depth);
            write_pfm(dir + "/sigma_" + tag + ".pfm", X, Y, sigma);
        } catch (const std::exception &e) {
            return die(e.what());
        }
        return 0;
    };
    bool have_map = false;
    for (size_t i = 0; i < frames; i++) {
        const double *xi = &odometry[6 * i];
        if (rendered) {
            double xi_cam[6];
            VGCHECK(vg_mono_odom_compose(xi, xbc.data(), xi_cam));
            VGCHECK(vg_render_views(d.r, 1, xi_cam, d.img, nullptr, nullptr, nullptr, nullptr, nullptr));
        } else {
            HIPCHECK(hipMemcpy(d.img, images[i].px.data(), img, hipMemcpyHostToDevice));
        }
        double report[VG_MONO_ODOM_REPORT], composed[6];
        VGCHECK(vg_mono_odom_feed_wheel_odometry(d.m, xi));
        VGCHECK(vg_mono_odom_feed_image(d.m, d.img, nullptr, report));
        VGCHECK(vg_mono_odom_xi_composed(d.m, composed));
        const int action = (int)report[2];
        trajectory += std::to_string(i) + " " + kStates[(int)report[1]] + " " + kActions[action];
        char buf[32];
        for (int k = 0; k < 7; k++) {
            trajectory += ' ';
            trajectory.append(buf, (size_t)vgtext::fmt_g6(k < 6 ? composed[k] : report[3], buf));
        }
        trajectory += '\n';
        if (action == VG_MONO_ODOM_SPARSE_INIT_KEYFRAME || action == VG_MONO_ODOM_KEYFRAME) {
            have_map = true;
            if (const int rc = write_map(std::to_string((long long)report[15] - 1))) return rc;
        }
        if (warp && have_map) {
            VGCHECK(vg_mono_odom_warp_image(d.m, d.img, nullptr, nullptr, d.warped));
            HIPCHECK(hipMemcpy(host.data(), d.warped, img, hipMemcpyDeviceToHost));
            try {
                write_pgm(dir + "/warp_" + std::to_string(i) + ".pgm", W, H, host.data());
            } catch (const std::exception &e) {
                return die(e.what());
            }
        }
    }
    if (have_map)
        if (const int rc = write_map("final")) return rc;
    try {
        write_file(dir + "/trajectory.txt", "", trajectory.data(), trajectory.size());
    } catch (const std::exception &e) {
        return die(e.what());
    }
    return 0;
}
