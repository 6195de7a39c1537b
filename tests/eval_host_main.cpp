// Stand-alone host driver of peclr_amd/csrc/procrustes.hpp, the numeric core of the pose_eval kernel, compiled as plain C++
// (tests/test_pose_eval_host.py builds and runs it; it is also the program to run under -fsanitize=address,undefined).
//
//   eval_host_main IN OUT
//   IN : int32 B, then gt [B][21][3] float64, then pred [B][21][3] float64 (raw, native byte order)
//   OUT: per sample 9 + 1 + 3 + 63 + 21 float64: rot_mat, scale, translation, y_transform, distance of y_transform to gt
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../peclr_amd/csrc/procrustes.hpp"

int main(int argc, char** argv) {
    using namespace peclr::procrustes;
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) {
        std::perror(argv[1]);
        return 1;
    }
    int32_t B = 0;
    if (std::fread(&B, sizeof B, 1, in) != 1 || B <= 0 || B > (1 << 20)) {
        std::fprintf(stderr, "bad sample count\n");
        std::fclose(in);
        return 1;
    }
    const size_t n = (size_t)B * kJoints * 3;
    std::vector<double> gt(n), pred(n);
    const bool ok = std::fread(gt.data(), sizeof(double), n, in) == n && std::fread(pred.data(), sizeof(double), n, in) == n;
    std::fclose(in);
    if (!ok) {
        std::fprintf(stderr, "short input\n");
        return 1;
    }
    constexpr int kPer = 9 + 1 + 3 + kJoints * 3 + kJoints;
    std::vector<double> out((size_t)B * kPer);
    for (int b = 0; b < B; ++b) {
        const double(*X)[3] = reinterpret_cast<const double(*)[3]>(gt.data() + (size_t)b * kJoints * 3);
        const double(*Y)[3] = reinterpret_cast<const double(*)[3]>(pred.data() + (size_t)b * kJoints * 3);
        Fit f;
        fit(X, Y, kJoints, f);
        double* o = out.data() + (size_t)b * kPer;
        for (int i = 0; i < 9; ++i) o[i] = f.R[i / 3][i % 3];
        o[9] = f.scale;
        for (int i = 0; i < 3; ++i) o[10 + i] = f.t[i];
        double(*al)[3] = reinterpret_cast<double(*)[3]>(o + 13);
        transform_cloud(f, Y, kJoints, al);
        for (int j = 0; j < kJoints; ++j) o[13 + kJoints * 3 + j] = joint_distance(al[j], X[j], 3);
    }
    std::FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) {
        std::perror(argv[2]);
        return 1;
    }
    const bool wrote = std::fwrite(out.data(), sizeof(double), out.size(), fo) == out.size();
    std::fclose(fo);
    return wrote ? 0 : 1;
}
