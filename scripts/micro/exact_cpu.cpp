// exact_cpu.cpp -- the CPU yardstick of uavhip_solve_exact (scripts/exact_bench.py builds and runs it):
// the subset DP of include/uavhip.h, unconstrained, with the (T - 1) & S submask walk, OpenMP over the
// states. Input file: int32 N, M, S; double omega; per scene P [N][M], v [M], c [N] (doubles).
// Output: one line "J <optimum>" per scene, then "seconds_per_scene <mean>".   g++ -O2 -fopenmp
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    int h[3];
    double w;
    if (!f || fread(h, 4, 3, f) != 3 || fread(&w, 8, 1, f) != 1 || h[0] < 1 || h[0] > 20) return 1;
    const int N = h[0], M = h[1], S = h[2], F = 1 << N;
    std::vector<double> P(N * M), v(M), c(N), val(F), D(F), E(F);
    double total = 0;
    for (int s = 0; s < S; ++s) {
        if (fread(P.data(), 8, N * M, f) != (size_t)(N * M) || fread(v.data(), 8, M, f) != (size_t)M ||
            fread(c.data(), 8, N, f) != (size_t)N) return 1;
        const auto t0 = std::chrono::steady_clock::now();
        std::fill(D.begin(), D.end(), 0.0);
        for (int t = 0; t < M; ++t) {
#pragma omp parallel for schedule(dynamic, 256)
            for (int T = 0; T < F; ++T) {
                double q = 1, cs = 0;
                for (int u = 0; u < N; ++u)
                    if (T >> u & 1) q *= 1 - P[u * M + t], cs += c[u];
                val[T] = v[t] * (1 - q) - w * cs;
            }
#pragma omp parallel for schedule(dynamic, 64)
            for (int X = 0; X < F; ++X) {
                double best = D[X] + val[0];
                for (int T = X; T; T = (T - 1) & X) best = std::max(best, D[X ^ T] + val[T]);
                E[X] = best;
            }
            D.swap(E);
        }
        total += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("J %.17g\n", D[F - 1]);
    }
    printf("seconds_per_scene %.6f\n", total / S);
    return 0;
}
