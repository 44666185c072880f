// search_multistart.hip -- the best of R restarts of the constrained exchange-move search per row
// (uavhip_search_multistart, and uavhip_search_multistart_from with R0 given starts per row). The rule is
// in include/uavhip.h. Built with -ffp-contract=off: the tests compare every replica bit for bit with a
// Python restatement of the rule, and the given replicas with k_search_constrained.
//
// Two launches on a caller-owned workspace, no LDS, no atomics, no grid-wide synchronisation:
//   k_search_multistart: one wave per (row s, replica r), four per workgroup, S * R waves, wave s * R + r
//       -- k_search_constrained's shape and its five instantiations, and its code: RefineRow<.., LIM = true>
//       (refine_device.hpp), start_limits and best_exchange (search_device.hpp), the loop of
//       search_loop_body.hpp. What is new is the start. The row has R0 given starts [R0][N]: lane u of
//       replica r < R0 converts its own id of start r, or of start 0 when UAV u is fixed, so every replica
//       holds the fixed UAVs where start 0 puts them; a replica r >= R0 converts start 0 and then lane
//       u < N, unless UAV u is fixed, draws its list index from one Philox4x32-10 block per four UAVs.
//       uavhip_search_multistart is R0 = 1, one kernel for both entry points. A replica's J,
//       covered, ids and eight counters go to the workspace, written by RefineRow::finish itself with
//       the wave's index for the row.
//   k_multistart_select: one wave per row. Lane l walks replicas l, l + 64, ...: the largest J with the
//       lowest r (strict >), the replicas above replica 0's J counted; a six-step butterfly (wave_argmax:
//       the lowest r among equal J) and a sum; then the chosen replica's results are copied out and,
//       when asked for, all R values of J. The kernel boundary is the dependence between the two, so
//       assignment_out may alias the one given start of R0 = 1.
// Workspace of W = S * R waves: J [W] f64 | assignment [W][N] i32 | covered [W] i32 | stats [W][8] i32.
#include "search_device.hpp"

namespace uavhip {
namespace {

struct MultistartLayout {
    long long a_off, cov_off, stats_off, bytes;  // J at 0
};
inline MultistartLayout multistart_layout(long long W, int N) {
    MultistartLayout l;
    l.a_off = 8 * W;
    l.cov_off = l.a_off + 4 * W * N;
    l.stats_off = l.cov_off + 4 * W;
    l.bytes = (l.stats_off + 32 * W + 15) & ~15ll;
    return l;
}

template <int TPL, int NR>
__global__ __launch_bounds__(64 * kRefineWaves) void k_search_multistart(
    uavhip_env env, int stride, int S, int R, int R0, uint32_t key0, uint32_t key1, int max_exchanges, int max_sweeps,
    const uint8_t* __restrict__ allowed, const uint8_t* __restrict__ fixed, const int* __restrict__ capacity,
    const int* __restrict__ starts, int* __restrict__ wa, double* __restrict__ wJ, int* __restrict__ wcov,
    int* __restrict__ wstats) {
    const int w = blockIdx.x * kRefineWaves + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (w >= S * R) return;  // S * R <= 2^30: the entry point refuses more
    const int s = w / R, rep = w - s * R;
    RefineRow<TPL, NR, true> r;
    r.load(env, s, stride, lane);
    const bool fx = fixed && r.isu && fixed[(long long)s * r.N + lane];
    // the lane's id is starts[s][k][lane], k = the replica's own start for a free UAV of a given replica,
    // else start 0; RefineRow::convert adds s * N + lane itself. It counts what the lanes hold, so
    // `invalid` is that of the start the replica is actually given.
    const int k = rep < R0 && !fx ? rep : 0;
    r.convert(starts ? starts + ((long long)s * (R0 - 1) + k) * r.N : nullptr, s);
    if (rep >= R0) {
        // a list index per free UAV: word u & 3 of the block of counter {u >> 2, rep, s, "STRM"}
        const u32x4 x = philox(u32x4{(uint32_t)lane >> 2, (uint32_t)rep, (uint32_t)s, 0x5354524Du}, key0, key1);
        const uint32_t word = (lane & 2) ? ((lane & 1) ? x.w : x.z) : ((lane & 1) ? x.y : x.x);
        if (r.isu && !fx) r.a = (int)(((unsigned long long)word * (uint32_t)r.M) >> 32);
    }
    int dropped, conflicts;
    start_limits(r, s, allowed, fixed, capacity, dropped, conflicts);
    r.load_columns();
#include "search_loop_body.hpp"

    r.finish(w, wa, wJ, wcov);
    if (lane < 8) wstats[(long long)w * 8 + lane] = search_stat(r, lane, exchanges, scan_clean, dropped, conflicts);
}

__global__ __launch_bounds__(64 * kRefineWaves) void k_multistart_select(
    int S, int R, int N, const int* __restrict__ wa, const double* __restrict__ wJ, const int* __restrict__ wcov,
    const int* __restrict__ wstats, int* __restrict__ aout, double* __restrict__ J, int* __restrict__ covered,
    int* __restrict__ stats, double* __restrict__ J_all) {
    const int s = blockIdx.x * kRefineWaves + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (s >= S) return;
    const long long w0 = (long long)s * R;
    const double J0 = wJ[w0];
    double bJ = -__builtin_huge_val();
    int br = 0x7fffffff, above = 0;
    for (int r = lane; r < R; r += kWave) {
        const double Jr = wJ[w0 + r];
        if (J_all) J_all[w0 + r] = Jr;
        above += Jr > J0;
        if (Jr > bJ) {
            bJ = Jr;
            br = r;
        }
    }
    wave_argmax(bJ, br);
    br = readlane_i(br, 0);
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) above += __shfl_xor(above, m);
    if (br >= R) br = 0;  // no J compared greater than -inf (NaN tables): replica 0, and an index inside the workspace
    const long long wb = w0 + br;
    if (lane < N) aout[(long long)s * N + lane] = wa[wb * N + lane];
    if (lane == 0) {
        J[s] = wJ[wb];
        covered[s] = wcov[wb];
    }
    if (stats && lane < 10) stats[(long long)s * 10 + lane] = lane < 8 ? wstats[wb * 8 + lane] : lane == 8 ? br : above;
}

}  // namespace
}  // namespace uavhip

extern "C" int64_t uavhip_multistart_workspace_bytes(int32_t S, int32_t R, int32_t N) {
    if (S < 1 || R < 1 || R > UAVHIP_MULTISTART_MAX_R || N < 1 || N > UAVHIP_MAX_N || (long long)S * R > (1ll << 30))
        return -1;
    return uavhip::multistart_layout((long long)S * R, N).bytes;
}

namespace uavhip {
namespace {

// both entry points: uavhip_search_multistart is R0 = 1 with its assignment_in for `starts`
int multistart_launch(const char* fn, const uavhip_env* env, int32_t env_stride, int32_t S, int32_t R, int32_t R0,
                      uint64_t seed, int32_t max_exchanges, int32_t max_sweeps, const uint8_t* allowed,
                      const uint8_t* fixed, const int32_t* capacity, const int32_t* starts, int32_t* assignment_out,
                      double* J, int32_t* covered, int32_t* stats, double* J_all, void* workspace,
                      int64_t workspace_bytes, uavhip_stream_t stream) {
    if (const int rc = check_rows(fn, env, env_stride, S,
                                  max_exchanges >= 0 && max_sweeps >= 0 && R >= 1 && R <= UAVHIP_MULTISTART_MAX_R &&
                                      assignment_out && J && covered,
                                  "max_exchanges=%d >= 0, max_sweeps=%d >= 0, 1 <= R=%d <= %d", max_exchanges,
                                  max_sweeps, R, UAVHIP_MULTISTART_MAX_R))
        return rc;
    if (R0 < 1 || R0 > R || (!starts && R0 > 1)) {
        set_error("%s: need 1 <= R0=%d <= R=%d given starts, and starts=%p non-NULL when R0 > 1 (NULL is the one "
                  "empty start of R0 == 1)", fn, R0, R, (const void*)starts);
        return UAVHIP_EINVAL;
    }
    const int64_t need = uavhip_multistart_workspace_bytes(S, R, env->N);
    if (need < 0 || !workspace || ((uintptr_t)workspace & 15) || workspace_bytes < need) {
        set_error("%s: workspace=%p (16-byte aligned) of %lld bytes: S=%d rows x R=%d replicas of N=%d need %lld "
                  "(uavhip_multistart_workspace_bytes; < 0: S * R > 2^30)", fn, workspace, (long long)workspace_bytes,
                  S, R, env->N, (long long)need);
        return UAVHIP_EINVAL;
    }
    const long long W = (long long)S * R;
    const MultistartLayout l = multistart_layout(W, env->N);
    char* ws = static_cast<char*>(workspace);
    double* wJ = reinterpret_cast<double*>(ws);
    int* wa = reinterpret_cast<int*>(ws + l.a_off);
    int* wcov = reinterpret_cast<int*>(ws + l.cov_off);
    int* wstats = reinterpret_cast<int*>(ws + l.stats_off);
    UAVHIP_ROWS_LAUNCH(env, (int)W, (k_search_multistart<TPL, NCAP>), stream, *env, (int)env_stride, (int)S, (int)R,
                       (int)R0, (uint32_t)seed, (uint32_t)(seed >> 32), (int)max_exchanges, (int)max_sweeps, allowed,
                       fixed, capacity, starts, wa, wJ, wcov, wstats);
    hipLaunchKernelGGL(k_multistart_select, dim3((S + kRefineWaves - 1) / kRefineWaves), dim3(64 * kRefineWaves), 0,
                       (hipStream_t)stream, (int)S, (int)R, (int)env->N, wa, wJ, wcov, wstats, assignment_out, J, covered,
                       stats, J_all);
    return check_launch("k_search_multistart");
}

}  // namespace
}  // namespace uavhip

extern "C" int uavhip_search_multistart(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t R, uint64_t seed,
                                        int32_t max_exchanges, int32_t max_sweeps, const uint8_t* allowed,
                                        const uint8_t* fixed, const int32_t* capacity, const int32_t* assignment_in,
                                        int32_t* assignment_out, double* J, int32_t* covered, int32_t* stats,
                                        double* J_all, void* workspace, int64_t workspace_bytes,
                                        uavhip_stream_t stream) {
    return uavhip::multistart_launch("uavhip_search_multistart", env, env_stride, S, R, 1, seed, max_exchanges,
                                     max_sweeps, allowed, fixed, capacity, assignment_in, assignment_out, J, covered,
                                     stats, J_all, workspace, workspace_bytes, stream);
}

extern "C" int uavhip_search_multistart_from(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t R,
                                             int32_t R0, uint64_t seed, int32_t max_exchanges, int32_t max_sweeps,
                                             const uint8_t* allowed, const uint8_t* fixed, const int32_t* capacity,
                                             const int32_t* starts, int32_t* assignment_out, double* J,
                                             int32_t* covered, int32_t* stats, double* J_all, void* workspace,
                                             int64_t workspace_bytes, uavhip_stream_t stream) {
    return uavhip::multistart_launch("uavhip_search_multistart_from", env, env_stride, S, R, R0, seed, max_exchanges,
                                     max_sweeps, allowed, fixed, capacity, starts, assignment_out, J, covered, stats,
                                     J_all, workspace, workspace_bytes, stream);
}
