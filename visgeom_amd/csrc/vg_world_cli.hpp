// vg_world_cli.hpp -- what the `mono_odom` and `mapping` programs share besides vg_stereo_cli.hpp: a pose from a transform literal
// and the world file of the `render` program, read without its views.  Host only.
#pragma once

#include "vg_stereo_cli.hpp"

namespace vgcli {

inline std::vector<double> pose_of(const vgjson::Value &v, const std::string &what)
{
    const std::vector<double> values = v.as_vector();
    std::vector<double> xi(6);
    if (vg_transform_from_values((int)values.size(), values.data(), xi.data()) != VG_OK) throw std::runtime_error(what + ": " + vg_last_error());
    return xi;
}

struct World {
    int width = 0, height = 0;
    std::vector<Image> textures;
    std::vector<vg_render_object> objects;
};

// the world file of the `render` program, without its views
inline void read_world(const std::string &path, World &w)
{
    const std::string dir = dir_of(path);
    const vgjson::Value root = vgjson::parse_file(path);
    if (root.kind != vgjson::Value::Object) throw std::runtime_error(path + ": a JSON object expected");
    w.width = as_int(root.at("width"), "width");
    w.height = as_int(root.at("height"), "height");
    const vgjson::Value &bg = root.at("background"), &planes = root.at("planes");
    if (bg.kind != vgjson::Value::Object) throw std::runtime_error("background: an object expected");
    if (planes.kind != vgjson::Value::Array || planes.arr.size() > VG_RENDER_MAX_PLANES) throw std::runtime_error("planes: an array of at most 64 planes expected");
    w.textures.reserve(planes.arr.size() + 1);   // the objects point into it
    w.textures.push_back(read_pgm(resolve(dir, bg.at("image_name").as_string())));
    vg_render_object o = {};
    o.kind = VG_RENDER_BACKGROUND;
    w.objects.push_back(o);
    for (size_t i = 0; i < planes.arr.size(); i++) {
        const vgjson::Value &p = planes.arr[i];
        const std::string what = "planes[" + std::to_string(i) + "]";
        if (p.kind != vgjson::Value::Object) throw std::runtime_error(what + ": an object expected");
        w.textures.push_back(read_pgm(resolve(dir, p.at("image_name").as_string())));
        o = vg_render_object{};
        o.kind = VG_RENDER_PLANE;
        const std::vector<double> xi = pose_of(p.at("pose"), what + ".pose");
        for (int k = 0; k < 6; k++) o.pose[k] = xi[(size_t)k];
        o.width = p.at("width").as_number();
        o.height = p.at("height").as_number();
        w.objects.push_back(o);
    }
    for (size_t i = 0; i < w.objects.size(); i++) {
        w.objects[i].texture = w.textures[i].px.data();
        w.objects[i].cols = w.textures[i].w;
        w.objects[i].rows = w.textures[i].h;
    }
}

}  // namespace vgcli
