// hough -- the reference's hough_test (test/reconstruction/hough_test.cpp) on files:
//     hough lines.json
// reads the reference's keys "width", "height", "camera_params" (6 EUCM parameters), "acc_params" (the accumulator camera) and
// "names" (the images: binary 8-bit PGM of that size, paths relative to the JSON's directory).  For image k the program writes,
// next to the JSON, lines_<k>.txt (one line per detection: the 16 values of a line in %.17g and its status), acc_<k>.pgm (the
// blurred accumulator x 255 / 100, rounded half to even and saturated) and res_<k>.pgm (the image with every traced pixel set
// to 255).  Files, not windows; PGM, not PNG.  Everything is read and checked before the GPU is touched.
#include <cfenv>

#include "vg_stereo_cli.hpp"

using namespace vgcli;

int main(int argc, char **argv)
{
    program() = "hough";
    if (argc != 2) {
        std::fprintf(stderr, "usage: hough lines.json\n");
        return 2;
    }
    const std::string dir = dir_of(argv[1]);
    std::vector<double> cam, acc_cam;
    std::vector<unsigned char> images;   // [n][height][width]
    int width = 0, height = 0;
    size_t n = 0;
    try {
        const vgjson::Value root = vgjson::parse_file(argv[1]);
        if (root.kind != vgjson::Value::Object) throw std::runtime_error("a JSON object expected");
        width = as_int(root.at("width"), "width");
        height = as_int(root.at("height"), "height");
        cam = vec6(root, "camera_params");
        acc_cam = vec6(root, "acc_params");
        const vgjson::Value &names = root.at("names");
        if (names.kind != vgjson::Value::Array || names.arr.empty()) throw std::runtime_error("names: an array of at least one image expected");
        for (const vgjson::Value &name : names.arr) {
            const std::string path = resolve(dir, name.as_string());
            const Image im = read_pgm(path);
            if (im.w != width || im.h != height) throw std::runtime_error(path + ": the image is not width x height");
            images.insert(images.end(), im.px.begin(), im.px.end());
        }
        n = names.arr.size();
    } catch (const std::exception &e) {
        return die(std::string(argv[1]) + ": " + e.what());
    }

    struct Owned {   // released on every way out of main
        vg_hough *h = nullptr;
        unsigned char *img = nullptr;
        float *blur = nullptr;
        ~Owned()
        {
            vg_hough_destroy(h);
            (void)hipFree(img);
            (void)hipFree(blur);
        }
    } d;
    VGCHECK(vg_hough_create(&d.h, 0, nullptr, width, height, cam.data(), acc_cam.data(), nullptr));
    int acc_w = 0, acc_h = 0;
    VGCHECK(vg_hough_size(d.h, &acc_w, &acc_h));
    const size_t P = (size_t)width * height, bins = (size_t)acc_w * acc_h;
    const int max_lines = 1024;
    HIPCHECK(hipMalloc(&d.img, n * P));
    HIPCHECK(hipMalloc(&d.blur, n * bins * sizeof(float)));
    HIPCHECK(hipMemcpy(d.img, images.data(), n * P, hipMemcpyHostToDevice));
    std::vector<double> lines(n * max_lines * VG_HOUGH_LINE);
    std::vector<int32_t> status(n * max_lines), count(n);
    VGCHECK(vg_hough_detect(d.h, (int64_t)n, d.img, max_lines, lines.data(), status.data(), count.data(), d.blur));   // all images in one call
    std::vector<float> blur(n * bins);
    HIPCHECK(hipMemcpy(blur.data(), d.blur, n * bins * sizeof(float), hipMemcpyDeviceToHost));
    std::fesetround(FE_TONEAREST);
    std::vector<unsigned char> acc8(bins);
    std::vector<int32_t> uv(2 * VG_HOUGH_MAX_TRACE);
    for (size_t k = 0; k < n; k++) {
        const std::string tag = std::to_string(k);
        std::string text;
        unsigned char *res = images.data() + k * P;
        const int found = std::min(count[k], max_lines);
        if (count[k] > max_lines) std::fprintf(stderr, "hough: image %zu: %d lines found, the first %d written\n", k, count[k], max_lines);
        for (int j = 0; j < found; j++) {
            const double *L = lines.data() + (k * max_lines + (size_t)j) * VG_HOUGH_LINE;
            char buf[32];
            for (int i = 0; i < VG_HOUGH_LINE; i++) {
                std::snprintf(buf, sizeof buf, "%.17g ", L[i]);
                text += buf;
            }
            text += std::to_string(status[k * max_lines + (size_t)j]) + "\n";
            if (status[k * max_lines + (size_t)j] != VG_HOUGH_OK) continue;
            int steps = 0;
            VGCHECK(vg_hough_trace(L + 6, L + 12, VG_HOUGH_MAX_TRACE, uv.data(), &steps));
            for (int i = 0; i < steps; i++) {
                const int u = uv[2 * (size_t)i], v = uv[2 * (size_t)i + 1];
                if (u >= 0 && u < width && v >= 0 && v < height) res[(size_t)v * width + u] = 255;   // the reference writes unchecked
            }
        }
        for (size_t i = 0; i < bins; i++) {
            const float x = std::nearbyint(blur[k * bins + i] * 255.f / 100.f);
            acc8[i] = (unsigned char)(x < 0.f ? 0.f : (x > 255.f ? 255.f : x));
        }
        try {
            write_file(dir + "/lines_" + tag + ".txt", text, nullptr, 0);
            write_pgm(dir + "/acc_" + tag + ".pgm", acc_w, acc_h, acc8.data());
            write_pgm(dir + "/res_" + tag + ".pgm", width, height, res);
        } catch (const std::exception &e) {
            return die(e.what());
        }
    }
    return 0;
}
