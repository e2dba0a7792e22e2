// mapping -- the reference's two photometric mapping programs (test/localization/map_test.cpp, map_real_data.cpp) on files:
//     mapping sequence.json
// reads what PhotometricMapping(ptree) reads -- "xi_base_camera", "camera_params", "stereo_parameters" and "mapping_parameters"
// (MappingParameters(ptree): new_kf_distance_thresh and new_kf_angular_thresh are squared; the fields that are literals in the
// reference may be given too) -- and exactly one of two inputs:
//   rendered, as map_test.cpp   "render": the path of a world file as the `render` program reads it, and "program": [{"initial",
//                     "trajectory": [{"increment", "step_count"}, ...]}, ...].  Every program is one pass: reinit(initial), then
//                     for every step of every trajectory entry the pose xi advances by the increment and the wheel odometry
//                     by the increment plus "odometry_drift" (six numbers added to the increment, default [0, 0, 0, 0, 0.005,
//                     0]); steps whose index within their entry is no multiple of "frame_stride" (default 2) are skipped, the
//                     others are rendered at xi o xi_base_camera and fed.  A pass may carry "gain" and "offset" (ours): its
//                     images become gain * v + offset, rounded and saturated -- a second pass with another exposure.  The
//                     reference's unseeded random noise on the rendered pose is not reproduced: the ground truth is xi.
//   files, as map_real_data.cpp   "map_files": [file, ...], each a JSON with "gt": [pose, ...] and "names": [PGM, ...], fed to
//                     construct_map at xiMap^-1 o gt (xiMap: the first pose of the first map file), and "trajectory_files":
//                     [file, ...], each with "odom", "gt" and "names": a trajectory starts at the first frame for which
//                     select_frame(xiMap^-1 o gt) succeeds (reinit there), and again after the loop has gone to SLAM.  Either
//                     list may be empty.  Poses are transform literals, paths are relative to the file that names them.
// Optional keys of ours: "maps": true, "err": true, "save_map": directory, "load_map": directory (read through add_frame before
// anything else).  Writes next to the JSON: vo.txt (xi_inter o xi_local), wo.txt (the wheel odometry) and gt.txt, one pose per
// fed frame in the reference's number format; kf<k>.txt per pass -- rendered: the map's poses after pass k, files: "i       pose"
// for the frames of trajectory k after which the state is SLAM; frames.txt, one line per fed frame: pass, index, state, action,
// warning, map index, frames in the map and the three alignment sums of the frame against the inter frame (zeros without a
// map).  With "maps", depth_<n>.pfm for every fed frame n that made a new inter frame, and depth_final.pfm; with "err",
// err_<n>.pgm for every fed frame with a map; with "save_map", frame_<k>.pgm and poses.txt (17 significant digits) of the map at
// the end.  Everything is read and checked before the GPU is touched.
#include <sys/stat.h>

#include "vg_stereo_cli.hpp"
#include "vg_text_format.hpp"
#include "vg_world_cli.hpp"

using namespace vgcli;

namespace {

const char *const kStates[] = {"BEGIN", "INIT", "LOCALIZE", "SLAM"};
const char *const kWarnings[] = {"NONE", "SCALE", "ROTATION"};
const char *const kActions[] = {"FIRST", "WAITING", "INIT_SLAM", "INIT_LOCALIZE", "LOCALIZE_REFINED", "LOCALIZE_INTER_FRAME", "LOCALIZE_MAP_FRAME_CHANGED",
                                "LOCALIZE_MAP_FRAME_KEPT", "LOCALIZE_LEFT_MAP", "SLAM_REFINED", "SLAM_INTER_FRAME", "SLAM_ENTERED_MAP"};

struct Frame {   // one frame to feed
    std::vector<double> odom, gt;   // wheel odometry; ground truth (in the map's frame)
    int image = -1;                 // files: index into the images
    int index = 0;                  // files: position in its trajectory file
};

struct Pass {
    bool has_initial = false;       // rendered: reinit(initial) in front of the pass
    std::vector<double> initial;
    double gain = 1., offset = 0.;
    bool exposure = false;
    std::vector<Frame> frames;
};

struct MapFrame {
    std::vector<double> xi;
    int image;
};

// operator<<(Transformation): the translation and the rotation vector, each as Eigen prints a row vector
void append_pose(std::string &out, const double *xi)
{
    vgtext::fmt_vec_append(out, xi, 3);
    out += ' ';
    vgtext::fmt_vec_append(out, xi + 3, 3);
}

std::vector<double> compose(const std::vector<double> &a, const std::vector<double> &b)
{
    std::vector<double> r(6);
    if (vg_mono_odom_compose(a.data(), b.data(), r.data()) != VG_OK) throw std::runtime_error(vg_last_error());
    return r;
}

std::vector<double> in_frame(const std::vector<double> &base, const std::vector<double> &xi)
{
    std::vector<double> r(6);
    if (vg_transform_inverse_compose(base.data(), xi.data(), r.data()) != VG_OK) throw std::runtime_error(vg_last_error());
    return r;
}

bool flag(const vgjson::Value &root, const char *key)
{
    if (!root.has(key)) return false;
    if (root.at(key).kind != vgjson::Value::Bool) throw std::runtime_error(std::string(key) + ": true or false expected");
    return root.at(key).as_bool();
}

int load_image(std::vector<Image> &images, const std::string &path, const vg_stereo_params &p)
{
    images.push_back(read_pgm(path));
    if (images.back().w != p.u_max || images.back().h != p.v_max) throw std::runtime_error(path + ": the image size differs from uMax x vMax");
    return (int)images.size() - 1;
}

}  // namespace

int main(int argc, char **argv)
{
    program() = "mapping";
    if (argc != 2) {
        std::fprintf(stderr, "usage: mapping sequence.json\n");
        return 2;
    }
    const std::string dir = dir_of(argv[1]);
    std::vector<double> cam, xbc;
    std::vector<Image> images;          // files mode, and a loaded map
    std::vector<MapFrame> loaded, built;   // "load_map"; "map_files"
    std::vector<Pass> passes;
    World world;
    bool rendered = false, maps = false, err = false;
    std::string save_dir;
    vg_mapping_params mp;
    vg_mapping_params_default(&mp);
    vg_stereo_params &p = mp.motion.stereo;
    try {
        const vgjson::Value root = vgjson::parse_file(argv[1]);
        if (root.kind != vgjson::Value::Object) throw std::runtime_error("a JSON object expected");
        cam = vec6(root, "camera_params");
        xbc = pose_of(root.at("xi_base_camera"), "xi_base_camera");
        read_motion_stereo_parameters(root.at("stereo_parameters"), mp.motion);
        if (root.has("mapping_parameters")) {
            const vgjson::Value &m = root.at("mapping_parameters");
            if (m.kind != vgjson::Value::Object) throw std::runtime_error("mapping_parameters: an object expected");
            for (const auto &kv : m.obj) {
                const std::string &k = kv.first;
                if (k == "new_kf_distance_thresh") mp.new_kf_distance_thresh = std::pow(kv.second.as_number(), 2);
                else if (k == "new_kf_angular_thresh") mp.new_kf_angular_thresh = std::pow(kv.second.as_number(), 2);
                else if (k == "min_init_dist") mp.min_init_dist = kv.second.as_number();
                else if (k == "min_stereo_base") mp.min_stereo_base = kv.second.as_number();
                else if (k == "dist_thresh") mp.dist_thresh = kv.second.as_number();
                else if (k == "normalize_scale") mp.normalize_scale = kv.second.as_bool() ? 1 : 0;
                else if (k == "rotation_tolerance") mp.rotation_tolerance = kv.second.as_number();
                else if (k == "min_scale_length") mp.min_scale_length = kv.second.as_number();
                else if (k == "min_scale_ratio") mp.min_scale_ratio = kv.second.as_number();
                else if (k == "max_scale_ratio") mp.max_scale_ratio = kv.second.as_number();
                else if (k == "num_scales") mp.num_scales = as_int(kv.second, k);
                else throw std::runtime_error("mapping_parameters: unknown key " + k);
            }
        }
        maps = flag(root, "maps");
        err = flag(root, "err");
        if (root.has("save_map")) save_dir = resolve(dir, root.at("save_map").as_string());
        rendered = root.has("render");
        if (rendered == (root.has("map_files") || root.has("trajectory_files")))
            throw std::runtime_error("exactly one of \"render\" and \"map_files\" / \"trajectory_files\" expected");
        if (root.has("load_map")) {
            const std::string from = resolve(dir, root.at("load_map").as_string());
            std::ifstream f(from + "/poses.txt");
            if (!f) throw std::runtime_error("cannot open " + from + "/poses.txt");
            std::vector<double> xi(6);
            for (int k = 0; f >> xi[0]; k++) {
                for (int i = 1; i < 6; i++)
                    if (!(f >> xi[(size_t)i])) throw std::runtime_error(from + "/poses.txt: six numbers per frame expected");
                loaded.push_back(MapFrame{xi, load_image(images, from + "/frame_" + std::to_string(k) + ".pgm", p)});
            }
        }
        if (rendered) {
            read_world(resolve(dir, root.at("render").as_string()), world);
            if (world.width != p.u_max || world.height != p.v_max) throw std::runtime_error("the world's image size differs from uMax x vMax");
            const int stride = root.has("frame_stride") ? as_int(root.at("frame_stride"), "frame_stride") : 2;
            if (stride < 1) throw std::runtime_error("frame_stride must be at least 1");
            std::vector<double> drift = {0., 0., 0., 0., 0.005, 0.};   // zetawo.rot()[1] += 0.005
            if (root.has("odometry_drift")) drift = root.at("odometry_drift").as_vector();
            if (drift.size() != 6) throw std::runtime_error("odometry_drift: six numbers expected");
            const vgjson::Value &prog = root.at("program");
            if (prog.kind != vgjson::Value::Array || prog.arr.empty()) throw std::runtime_error("program: a non-empty array expected");
            for (size_t n = 0; n < prog.arr.size(); n++) {
                const vgjson::Value &x = prog.arr[n];
                const std::string what = "program[" + std::to_string(n) + "]";
                if (x.kind != vgjson::Value::Object) throw std::runtime_error(what + ": an object expected");
                Pass pass;
                pass.has_initial = true;
                pass.initial = pose_of(x.at("initial"), what + ".initial");
                if (x.has("gain") || x.has("offset")) {
                    pass.exposure = true;
                    if (x.has("gain")) pass.gain = x.at("gain").as_number();
                    if (x.has("offset")) pass.offset = x.at("offset").as_number();
                    if (!std::isfinite(pass.gain) || !std::isfinite(pass.offset)) throw std::runtime_error(what + ": gain and offset must be finite");
                }
                std::vector<double> xi = pass.initial, xiwo = pass.initial;
                const vgjson::Value &tr = x.at("trajectory");
                if (tr.kind != vgjson::Value::Array) throw std::runtime_error(what + ".trajectory: an array expected");
                for (const vgjson::Value &it : tr.arr) {
                    if (it.kind != vgjson::Value::Object) throw std::runtime_error(what + ".trajectory: objects expected");
                    const std::vector<double> zeta = pose_of(it.at("increment"), what + ".increment");
                    std::vector<double> zetawo(6);
                    for (int i = 0; i < 6; i++) zetawo[(size_t)i] = zeta[(size_t)i] + drift[(size_t)i];
                    const int steps = as_int(it.at("step_count"), what + ".step_count");
                    if (steps < 0 || steps > 65535) throw std::runtime_error(what + ".step_count must be in [0, 65535]");
                    for (int i = 0; i < steps; i++, xi = compose(xi, zeta), xiwo = compose(xiwo, zetawo)) {
                        if (i % stride) continue;
                        Frame f;
                        f.odom = xiwo;
                        f.gt = xi;
                        pass.frames.push_back(f);
                    }
                }
                passes.push_back(pass);
            }
        } else {
            std::vector<double> xi_map;
            auto poses_of = [&](const vgjson::Value &doc, const char *key, const std::string &file) {
                const vgjson::Value &a = doc.at(key);
                if (a.kind != vgjson::Value::Array) throw std::runtime_error(file + ": " + key + ": an array expected");
                std::vector<std::vector<double>> out;
                for (size_t i = 0; i < a.arr.size(); i++) out.push_back(pose_of(a.arr[i], file + ": " + key + "[" + std::to_string(i) + "]"));
                return out;
            };
            auto names_of = [&](const vgjson::Value &doc, const std::string &file, size_t want) {
                const vgjson::Value &a = doc.at("names");
                if (a.kind != vgjson::Value::Array || a.arr.size() != want) throw std::runtime_error(file + ": one name per pose expected");
                std::vector<int> out;
                for (const vgjson::Value &v : a.arr) out.push_back(load_image(images, resolve(dir_of(file), v.as_string()), p));
                return out;
            };
            vgjson::Value empty_list;
            empty_list.kind = vgjson::Value::Array;
            const vgjson::Value &mf = root.has("map_files") ? root.at("map_files") : empty_list;
            const vgjson::Value &tf = root.has("trajectory_files") ? root.at("trajectory_files") : empty_list;
            if (mf.kind != vgjson::Value::Array || tf.kind != vgjson::Value::Array) throw std::runtime_error("map_files, trajectory_files: arrays expected");
            for (const vgjson::Value &name : mf.arr) {
                const std::string file = resolve(dir, name.as_string());
                const vgjson::Value doc = vgjson::parse_file(file);
                const auto gt = poses_of(doc, "gt", file);
                const auto img = names_of(doc, file, gt.size());
                if (xi_map.empty() && !gt.empty()) xi_map = gt[0];
                for (size_t i = 0; i < gt.size(); i++) built.push_back(MapFrame{in_frame(xi_map, gt[i]), img[i]});
            }
            if (xi_map.empty()) xi_map.assign(6, 0.);   // no map file: the trajectories' ground truth is in the map's frame already
            for (const vgjson::Value &name : tf.arr) {
                const std::string file = resolve(dir, name.as_string());
                const vgjson::Value doc = vgjson::parse_file(file);
                const auto gt = poses_of(doc, "gt", file), odom = poses_of(doc, "odom", file);
                if (odom.size() != gt.size()) throw std::runtime_error(file + ": one odometry pose per ground truth pose expected");
                const auto img = names_of(doc, file, gt.size());
                Pass pass;
                for (size_t i = 0; i < gt.size(); i++) {
                    Frame f;
                    f.odom = odom[i];
                    f.gt = in_frame(xi_map, gt[i]);
                    f.image = img[i];
                    f.index = (int)i;
                    pass.frames.push_back(f);
                }
                passes.push_back(pass);
            }
        }
    } catch (const std::exception &e) {
        return die(std::string(argv[1]) + ": " + e.what());
    }

    struct Owned {   // released on every way out of main
        vg_mapping *m = nullptr;
        vg_render *r = nullptr;
        unsigned char *img = nullptr, *out = nullptr;
        ~Owned()
        {
            vg_mapping_destroy(m);
            vg_render_destroy(r);
            (void)hipFree(img);
            (void)hipFree(out);
        }
    } d;
    VGCHECK(vg_mapping_create(&d.m, 0, nullptr, cam.data(), xbc.data(), p.u_max, p.v_max, &mp));
    if (rendered) VGCHECK(vg_render_create(&d.r, 0, nullptr, cam.data(), world.width, world.height, (int)world.objects.size(), world.objects.data()));
    int W = 0, H = 0, X = 0, Y = 0;
    VGCHECK(vg_mapping_size(d.m, &W, &H, &X, &Y));
    const size_t img = (size_t)W * H, P = (size_t)X * Y;
    HIPCHECK(hipMalloc(&d.img, img));
    HIPCHECK(hipMalloc(&d.out, img));
    std::vector<double> depth(P);
    std::vector<unsigned char> host(img);
    std::string vo, wo, gt, lines;
    auto write_map = [&](const std::string &tag) -> int {
        const double *dd = nullptr, *ds = nullptr, *dc = nullptr;
        VGCHECK(vg_mapping_map(d.m, &dd, &ds, &dc));
        HIPCHECK(hipMemcpy(depth.data(), dd, P * sizeof(double), hipMemcpyDeviceToHost));
        try {
            write_pfm(dir + "/depth_" + tag + ".pfm", X, Y, depth);
        } catch (const std::exception &e) {
            return die(e.what());
        }
        return 0;
    };
    auto upload = [&](int image) -> int {
        HIPCHECK(hipMemcpy(d.img, images[(size_t)image].px.data(), img, hipMemcpyHostToDevice));
        return 0;
    };
    for (const MapFrame &f : loaded) {
        if (const int rc = upload(f.image)) return rc;
        VGCHECK(vg_mapping_add_frame(d.m, f.xi.data(), d.img));
    }
    for (const MapFrame &f : built) {
        if (const int rc = upload(f.image)) return rc;
        int inserted = 0;
        VGCHECK(vg_mapping_construct_map(d.m, f.xi.data(), d.img, &inserted));
    }
    bool have_map = false;
    long long fed = 0;
    for (size_t n = 0; n < passes.size(); n++) {
        const Pass &pass = passes[n];
        std::string kf;
        if (pass.has_initial) VGCHECK(vg_mapping_reinit(d.m, pass.initial.data()));
        bool initialized = pass.has_initial;
        for (const Frame &f : pass.frames) {
            if (!initialized) {   // files: find the starting point
                int idx = -1;
                VGCHECK(vg_mapping_select_frame(d.m, f.gt.data(), 4., &idx));
                if (idx == -1) continue;
                VGCHECK(vg_mapping_reinit(d.m, f.gt.data()));
                initialized = true;
            }
            if (rendered) {
                double xi_cam[6];
                VGCHECK(vg_mono_odom_compose(f.gt.data(), xbc.data(), xi_cam));
                VGCHECK(vg_render_views(d.r, 1, xi_cam, d.img, nullptr, nullptr, nullptr, nullptr, nullptr));
                if (pass.exposure) {
                    HIPCHECK(hipMemcpy(host.data(), d.img, img, hipMemcpyDeviceToHost));
                    for (unsigned char &v : host) {
                        const double e = std::floor(pass.gain * (double)v + pass.offset + 0.5);
                        v = (unsigned char)(e < 0. ? 0. : e > 255. ? 255. : e);
                    }
                    HIPCHECK(hipMemcpy(d.img, host.data(), img, hipMemcpyHostToDevice));
                }
            } else if (const int rc = upload(f.image)) {
                return rc;
            }
            double report[VG_MAPPING_REPORT], composed[6];
            VGCHECK(vg_mapping_feed_odometry(d.m, f.odom.data()));
            VGCHECK(vg_mapping_feed_image(d.m, d.img, nullptr, report));
            VGCHECK(vg_mapping_xi_composed(d.m, composed));
            append_pose(vo, composed);
            vo += '\n';
            append_pose(wo, f.odom.data());
            wo += '\n';
            append_pose(gt, f.gt.data());
            gt += '\n';
            const int state = (int)report[1], action = (int)report[2];
            const bool pushed = action != VG_MAPPING_FIRST && action != VG_MAPPING_WAITING && action != VG_MAPPING_LOCALIZE_REFINED && action != VG_MAPPING_SLAM_REFINED;
            have_map = have_map || pushed;
            int64_t sums[3] = {0, 0, 0};
            if (have_map) {
                VGCHECK(vg_mapping_alignment(d.m, nullptr, d.img, nullptr, nullptr, err ? d.out : nullptr, sums));
                if (err) {
                    HIPCHECK(hipMemcpy(host.data(), d.out, img, hipMemcpyDeviceToHost));
                    try {
                        write_pgm(dir + "/err_" + std::to_string(fed) + ".pgm", W, H, host.data());
                    } catch (const std::exception &e) {
                        return die(e.what());
                    }
                }
            }
            lines += std::to_string(n) + " " + std::to_string(fed) + " " + kStates[state] + " " + kActions[action] + " " + kWarnings[(int)report[3]] + " " +
                     std::to_string((long long)report[5]) + " " + std::to_string((long long)report[30]) + " " + std::to_string((long long)sums[0]) + " " +
                     std::to_string((long long)sums[1]) + " " + std::to_string((long long)sums[2]) + "\n";
            if (maps && pushed)
                if (const int rc = write_map(std::to_string(fed))) return rc;
            if (!rendered && state == VG_MAPPING_SLAM) {
                kf += std::to_string(f.index) + "       ";
                append_pose(kf, composed);
                kf += '\n';
                initialized = false;
            }
            fed++;
        }
        if (rendered) {
            int64_t count = 0;
            VGCHECK(vg_mapping_num_frames(d.m, &count));
            for (int64_t k = 0; k < count; k++) {
                double xi[6];
                VGCHECK(vg_mapping_get_frame(d.m, k, xi, nullptr));
                append_pose(kf, xi);
                kf += '\n';
            }
        }
        try {
            write_file(dir + "/kf" + std::to_string(n) + ".txt", "", kf.data(), kf.size());
        } catch (const std::exception &e) {
            return die(e.what());
        }
    }
    if (maps && have_map)
        if (const int rc = write_map("final")) return rc;
    try {
        write_file(dir + "/vo.txt", "", vo.data(), vo.size());
        write_file(dir + "/wo.txt", "", wo.data(), wo.size());
        write_file(dir + "/gt.txt", "", gt.data(), gt.size());
        write_file(dir + "/frames.txt", "", lines.data(), lines.size());
    } catch (const std::exception &e) {
        return die(e.what());
    }
    if (!save_dir.empty()) {
        (void)mkdir(save_dir.c_str(), 0777);
        int64_t count = 0;
        VGCHECK(vg_mapping_num_frames(d.m, &count));
        std::string poses;
        for (int64_t k = 0; k < count; k++) {
            double xi[6];
            VGCHECK(vg_mapping_get_frame(d.m, k, xi, d.out));
            HIPCHECK(hipMemcpy(host.data(), d.out, img, hipMemcpyDeviceToHost));
            char buf[40];
            for (int i = 0; i < 6; i++) {
                std::snprintf(buf, sizeof buf, "%.17g", xi[i]);
                poses += buf;
                poses += i < 5 ? ' ' : '\n';
            }
            try {
                write_pgm(save_dir + "/frame_" + std::to_string(k) + ".pgm", W, H, host.data());
            } catch (const std::exception &e) {
                return die(e.what());
            }
        }
        try {
            write_file(save_dir + "/poses.txt", "", poses.data(), poses.size());
        } catch (const std::exception &e) {
            return die(e.what());
        }
    }
    return 0;
}
