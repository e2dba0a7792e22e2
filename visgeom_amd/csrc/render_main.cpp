// render -- the reference's RenderDevice on files:
//     render world.json
// reads the world as RenderDevice(ptree) and test/reconstruction/renderer_test.cpp read it: "width", "height", "camera_params"
// (6 EUCM parameters), "background": {"image_name"} and "planes": [{"image_name", "pose", "width", "height"}, ...]; a pose is a
// transform literal as the calibration front end reads it.  Textures are binary 8-bit PGM, paths relative to the JSON's directory.
// One key of ours: "views": [pose, ...], the camera poses in the world.  For view k the program writes img_<k>.pgm (the image)
// and depth_<k>.pfm (the range along every pixel's ray, 1e6 where nothing is hit) next to the JSON.
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

}  // namespace

int main(int argc, char **argv)
{
    program() = "render";
    if (argc != 2) {
        std::fprintf(stderr, "usage: render world.json\n");
        return 2;
    }
    const std::string dir = dir_of(argv[1]);
    std::vector<double> cam, views;   // views: [n][6]
    std::vector<Image> textures;
    std::vector<vg_render_object> objects;
    int width = 0, height = 0;
    try {
        const vgjson::Value root = vgjson::parse_file(argv[1]);
        if (root.kind != vgjson::Value::Object) throw std::runtime_error("a JSON object expected");
        width = as_int(root.at("width"), "width");
        height = as_int(root.at("height"), "height");
        cam = vec6(root, "camera_params");
        const vgjson::Value &bg = root.at("background"), &planes = root.at("planes"), &vs = root.at("views");
        if (bg.kind != vgjson::Value::Object) throw std::runtime_error("background: an object expected");
        if (planes.kind != vgjson::Value::Array) throw std::runtime_error("planes: an array expected");
        if (planes.arr.size() > VG_RENDER_MAX_PLANES) throw std::runtime_error("planes: at most 64 planes");
        if (vs.kind != vgjson::Value::Array || vs.arr.empty()) throw std::runtime_error("views: an array of at least one camera pose expected");
        textures.reserve(planes.arr.size() + 1);   // the objects point into it
        textures.push_back(read_pgm(resolve(dir, bg.at("image_name").as_string())));
        vg_render_object o = {};
        o.kind = VG_RENDER_BACKGROUND;
        objects.push_back(o);
        for (size_t i = 0; i < planes.arr.size(); i++) {
            const vgjson::Value &p = planes.arr[i];
            const std::string what = "planes[" + std::to_string(i) + "]";
            if (p.kind != vgjson::Value::Object) throw std::runtime_error(what + ": an object expected");
            textures.push_back(read_pgm(resolve(dir, p.at("image_name").as_string())));
            o = vg_render_object{};
            o.kind = VG_RENDER_PLANE;
            const std::vector<double> xi = pose_of(p.at("pose"), what + ".pose");
            for (int k = 0; k < 6; k++) o.pose[k] = xi[(size_t)k];
            o.width = p.at("width").as_number();
            o.height = p.at("height").as_number();
            objects.push_back(o);
        }
        for (size_t i = 0; i < objects.size(); i++) {
            objects[i].texture = textures[i].px.data();
            objects[i].cols = textures[i].w;
            objects[i].rows = textures[i].h;
        }
        for (size_t i = 0; i < vs.arr.size(); i++) {
            const std::vector<double> xi = pose_of(vs.arr[i], "views[" + std::to_string(i) + "]");
            views.insert(views.end(), xi.begin(), xi.end());
        }
    } catch (const std::exception &e) {
        return die(std::string(argv[1]) + ": " + e.what());
    }

    struct Owned {   // released on every way out of main
        vg_render *r = nullptr;
        unsigned char *img = nullptr;
        float *depth = nullptr;
        ~Owned()
        {
            vg_render_destroy(r);
            (void)hipFree(img);
            (void)hipFree(depth);
        }
    } d;
    VGCHECK(vg_render_create(&d.r, 0, nullptr, cam.data(), width, height, (int)objects.size(), objects.data()));
    const size_t P = (size_t)width * height, n = views.size() / 6;
    HIPCHECK(hipMalloc(&d.img, n * P));
    HIPCHECK(hipMalloc(&d.depth, n * P * sizeof(float)));
    VGCHECK(vg_render_views(d.r, (int64_t)n, views.data(), d.img, d.depth, nullptr, nullptr, nullptr, nullptr));   // all views in one call
    std::vector<unsigned char> img(n * P);
    std::vector<float> depth(n * P);
    HIPCHECK(hipMemcpy(img.data(), d.img, n * P, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(depth.data(), d.depth, n * P * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<double> depth64(P);
    for (size_t k = 0; k < n; k++) {
        for (size_t i = 0; i < P; i++) depth64[i] = depth[k * P + i];
        try {
            write_pgm(dir + "/img_" + std::to_string(k) + ".pgm", width, height, img.data() + k * P);
            write_pfm(dir + "/depth_" + std::to_string(k) + ".pfm", width, height, depth64);
        } catch (const std::exception &e) {
            return die(e.what());
        }
    }
    return 0;
}
