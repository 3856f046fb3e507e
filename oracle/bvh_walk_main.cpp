// Stand-alone driver of bvh_walk.cpp for a sanitizer build (`make -C oracle bvh_walk_asan`): reads one dump
//   int32 n_vertices, n_faces, n_rays; double vertices[3 n_vertices]; int32 faces[3 n_faces]; double origins[3 n_rays], dirs[3 n_rays]
// and runs the check with the brute-force loop finding the crossings.  Exit status 1 when a crossing is lost.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int pvt_bvh_walk_check(const double*, int, const int32_t*, int, const double*, const double*, int, const int32_t*,
                                  const int32_t*, const double*, int, double*, int64_t*, int32_t*, int64_t);

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) return 2;
    int32_t head[3];
    if (std::fread(head, sizeof(int32_t), 3, fp) != 3) return 2;
    std::vector<double> v(3 * (size_t)head[0]), o(3 * (size_t)head[2]), d(3 * (size_t)head[2]);
    std::vector<int32_t> f(3 * (size_t)head[1]);
    bool ok = std::fread(v.data(), sizeof(double), v.size(), fp) == v.size() && std::fread(f.data(), sizeof(int32_t), f.size(), fp) == f.size() &&
              std::fread(o.data(), sizeof(double), o.size(), fp) == o.size() && std::fread(d.data(), sizeof(double), d.size(), fp) == d.size();
    std::fclose(fp);
    if (!ok) return 2;
    double out[13];
    std::vector<int64_t> ptr((size_t)head[2] + 1);
    std::vector<int32_t> reached((size_t)head[2] * (size_t)head[1]);
    const int rc = pvt_bvh_walk_check(v.data(), head[0], f.data(), head[1], o.data(), d.data(), head[2], nullptr, nullptr, nullptr, -1, out,
                                      ptr.data(), reached.data(), (int64_t)reached.size());
    std::printf("%s: rc %d, %.0f crossings of %d rays, %.0f lost, least slack / pad %.4f, %.0f leaves reached\n", argv[1], rc, out[7], head[2],
                out[0], out[3], out[9]);
    return rc != 0 || out[0] != 0.0;
}
