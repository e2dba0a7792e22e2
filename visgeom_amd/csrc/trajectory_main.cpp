// trajectory -- the reference's test/calibration/trajectory.cpp on files:
//     trajectory plan.json
// reads the plan as that program does: "trajectory1", "trajectory2", ... (here up to 8) with "x_0", "y_0", "theta_0", "v", "w",
// "number_steps"; "camera_params" (6 EUCM parameters), "camera_width", "camera_height"; "quality_parameters" with "xiBaseCam",
// "xiOrigBoard", "turn_radius", "board": {"cols", "rows", "step"}, "min_camera_dist", "min_margin", "min_cell_size",
// "prior_variance", "feature_variance"; "optimize".  Keys of ours: "starts": [[5 T numbers], ...], further start points of the
// minimisation, and "views": true.  It prints the visual covariance at the reference's probe pose, the cost of the start with
// its terms and the parameters of the best start, and writes trajectory.json next to the plan: per trajectory the rows
// [x, y, theta] of its poses, the form a calibration file's odometry takes.  With "views" it writes points_<t>_<i>.pgm for
// pose i of trajectory t: the board's projected corners as the reference draws them.
// Everything is read and checked before the GPU is touched.
#include "vg_stereo_cli.hpp"

using namespace vgcli;

namespace {

std::vector<double> pose_of(const vgjson::Value &v, const std::string &what)
{
    const std::vector<double> values = v.as_vector();
    std::vector<double> xi(6);
    if (vg_transform_from_values((int)values.size(), values.data(), xi.data()) != VG_OK) throw std::runtime_error(what + ": " + vg_last_error());
    return xi;
}

void print_matrix(const double *m)
{
    for (int r = 0; r < 6; r++) {
        for (int c = 0; c < 6; c++) std::printf("%s%.6g", c ? " " : "", m[6 * r + c]);
        std::printf("\n");
    }
}

}  // namespace

int main(int argc, char **argv)
{
    program() = "trajectory";
    if (argc != 2) {
        std::fprintf(stderr, "usage: trajectory plan.json\n");
        return 2;
    }
    const std::string dir = dir_of(argv[1]);
    std::vector<double> cam, points;   // points: [n_starts][5 T], the plan's own start first
    std::vector<int> steps;
    vg_trajectory_quality q = {};
    int width = 0, height = 0;
    bool optimize = false, views = false;
    try {
        const vgjson::Value root = vgjson::parse_file(argv[1]);
        if (root.kind != vgjson::Value::Object) throw std::runtime_error("a JSON object expected");
        for (int t = 1; t <= VG_TRAJECTORY_MAX && root.has("trajectory" + std::to_string(t)); t++) {
            const std::string name = "trajectory" + std::to_string(t);
            const vgjson::Value &tr = root.at(name);
            if (tr.kind != vgjson::Value::Object) throw std::runtime_error(name + ": an object expected");
            for (const char *key : {"x_0", "y_0", "theta_0", "v", "w"}) points.push_back(tr.at(key).as_number());
            steps.push_back(as_int(tr.at("number_steps"), name + ".number_steps"));
        }
        if (steps.empty()) throw std::runtime_error("trajectory1: missing");
        cam = vec6(root, "camera_params");
        width = as_int(root.at("camera_width"), "camera_width");
        height = as_int(root.at("camera_height"), "camera_height");
        const vgjson::Value &qp = root.at("quality_parameters");
        if (qp.kind != vgjson::Value::Object) throw std::runtime_error("quality_parameters: an object expected");
        const std::vector<double> xc = pose_of(qp.at("xiBaseCam"), "xiBaseCam"), xb = pose_of(qp.at("xiOrigBoard"), "xiOrigBoard");
        const std::vector<double> prior = qp.at("prior_variance").as_vector();
        if (prior.size() != 6) throw std::runtime_error("prior_variance: 6 numbers expected");
        for (int k = 0; k < 6; k++) {
            q.xi_base_cam[k] = xc[(size_t)k];
            q.xi_orig_board[k] = xb[(size_t)k];
            q.prior_variance[k] = prior[(size_t)k];
        }
        q.turn_radius = qp.at("turn_radius").as_number();
        const vgjson::Value &board = qp.at("board");
        q.board_cols = as_int(board.at("cols"), "board.cols");
        q.board_rows = as_int(board.at("rows"), "board.rows");
        q.board_step = board.at("step").as_number();
        q.min_camera_dist = qp.at("min_camera_dist").as_number();
        q.min_margin = qp.at("min_margin").as_number();
        q.min_cell_size = qp.at("min_cell_size").as_number();
        q.feature_variance = qp.at("feature_variance").as_number();
        optimize = root.at("optimize").as_bool();
        views = root.has("views") && root.at("views").as_bool();
        if (root.has("starts")) {
            const vgjson::Value &st = root.at("starts");
            if (st.kind != vgjson::Value::Array) throw std::runtime_error("starts: an array of parameter points expected");
            for (size_t i = 0; i < st.arr.size(); i++) {
                const std::vector<double> p = st.arr[i].as_vector();
                if (p.size() != steps.size() * VG_TRAJECTORY_PARAMS) throw std::runtime_error("starts[" + std::to_string(i) + "]: 5 numbers per trajectory expected");
                points.insert(points.end(), p.begin(), p.end());
            }
        }
    } catch (const std::exception &e) {
        return die(std::string(argv[1]) + ": " + e.what());
    }
    const int T = (int)steps.size(), PT = VG_TRAJECTORY_PARAMS * T;
    const int64_t n_starts = (int64_t)points.size() / PT;

    struct Owned {   // released on every way out of main
        vg_trajectory *h = nullptr;
        ~Owned() { vg_trajectory_destroy(h); }
    } d;
    VGCHECK(vg_trajectory_create(&d.h, 0, nullptr, VG_MODEL_EUCM, cam.data(), width, height, &q, T, steps.data()));

    // "Test the visual covariance": the camera of a robot at (0.1, 0.1, 0, 0, 0, 0.1)
    const double probe_base[6] = {0.1, 0.1, 0., 0., 0., 0.1};
    double probe[6], cov[36], info[36];
    int32_t bad = 0;
    VGCHECK(vg_mono_odom_compose(probe_base, q.xi_base_cam, probe));
    VGCHECK(vg_trajectory_visual_cov(d.h, 1, probe, cov, info, &bad));
    std::printf("visual covariance at the probe pose%s\n", bad ? " (invalid)" : "");
    print_matrix(cov);
    double cost = 0., terms[VG_TRAJECTORY_TERMS];
    VGCHECK(vg_trajectory_evaluate(d.h, 1, points.data(), &cost, terms, &bad));
    std::printf("start cost %.10g  information %.10g  image limits %.10g  curvature %.10g  distance %.10g  normal %.10g  invalid poses %d\n", cost,
                terms[0], terms[1], terms[2], terms[3], terms[4], (int)bad);

    std::vector<double> best(points.begin(), points.begin() + PT);
    if (optimize) {
        std::vector<double> costs((size_t)n_starts);
        std::vector<int32_t> iterations((size_t)n_starts), termination((size_t)n_starts);
        VGCHECK(vg_trajectory_optimize(d.h, n_starts, points.data(), nullptr, costs.data(), iterations.data(), termination.data()));
        int64_t arg = 0;
        for (int64_t k = 0; k < n_starts; k++) {
            std::printf("start %lld: cost %.10g after %d iterations, termination %d\n", (long long)k, costs[(size_t)k], (int)iterations[(size_t)k],
                        (int)termination[(size_t)k]);
            if (costs[(size_t)k] < costs[(size_t)arg]) arg = k;
        }
        best.assign(points.begin() + arg * PT, points.begin() + (arg + 1) * PT);
        std::printf("best start %lld\n", (long long)arg);
    }
    for (int t = 0; t < T; t++) {
        for (int j = 0; j < VG_TRAJECTORY_PARAMS; j++) std::printf("%.10g   ", best[(size_t)(t * VG_TRAJECTORY_PARAMS + j)]);
        std::printf("\n");
    }

    int total = 0;
    for (int s : steps) total += s;
    std::vector<double> xi((size_t)total * 6);
    VGCHECK(vg_trajectory_poses(T, steps.data(), best.data(), xi.data(), nullptr));
    std::string out = "{\n";
    char row[128];
    for (int t = 0, o = 0; t < T; t++) {
        out += "    \"trajectory" + std::to_string(t + 1) + "\": [\n";
        for (int i = 0; i < steps[(size_t)t]; i++, o++) {
            std::snprintf(row, sizeof row, "        [%.17g, %.17g, %.17g]%s\n", xi[(size_t)o * 6], xi[(size_t)o * 6 + 1], xi[(size_t)o * 6 + 5],
                          i + 1 < steps[(size_t)t] ? "," : "");
            out += row;
        }
        out += t + 1 < T ? "    ],\n" : "    ]\n";
    }
    out += "}\n";
    try {
        write_file(dir + "/trajectory.json", out, nullptr, 0);
        if (views) {
            const int N = q.board_cols * q.board_rows;
            std::vector<double> uv((size_t)N * 2);
            std::vector<int32_t> ok((size_t)N);
            std::vector<unsigned char> img((size_t)width * height);
            for (int t = 0, o = 0; t < T; t++)
                for (int i = 0; i < steps[(size_t)t]; i++, o++) {
                    double cam_pose[6];
                    if (vg_mono_odom_compose(xi.data() + (size_t)o * 6, q.xi_base_cam, cam_pose) != VG_OK ||
                        vg_trajectory_project_board(VG_MODEL_EUCM, cam.data(), &q, cam_pose, uv.data(), ok.data()) != VG_OK)
                        return die(vg_last_error());
                    // white, the two top and the two bottom rows black, a cross of five pixels on every corner (those that leave
                    // the image are left out: the reference writes outside its buffer there)
                    std::fill(img.begin(), img.end(), (unsigned char)255);
                    for (int y = 0; y < height; y++)
                        if (y < 2 || y >= height - 2) std::fill(img.begin() + (size_t)y * width, img.begin() + (size_t)(y + 1) * width, (unsigned char)0);
                    for (int k = 0; k < N; k++) {
                        if (!ok[(size_t)k] || !(std::fabs(uv[(size_t)2 * k]) < 1e9) || !(std::fabs(uv[(size_t)2 * k + 1]) < 1e9)) continue;
                        const long u = std::lround(uv[(size_t)2 * k]), v = std::lround(uv[(size_t)2 * k + 1]);
                        const long du[5] = {0, 0, 0, -1, 1}, dv[5] = {0, -1, 1, 0, 0};
                        for (int m = 0; m < 5; m++)
                            if (u + du[m] >= 0 && u + du[m] < width && v + dv[m] >= 0 && v + dv[m] < height) img[(size_t)(v + dv[m]) * width + (u + du[m])] = 0;
                    }
                    write_pgm(dir + "/points_" + std::to_string(t + 1) + "_" + std::to_string(i) + ".pgm", width, height, img.data());
                }
        }
    } catch (const std::exception &e) {
        return die(e.what());
    }
    return 0;
}
