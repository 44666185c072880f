// search_constrained.hip -- the exchange-move local search under three constraints
// (uavhip_search_assignments_constrained): pairs that may not be flown (allowed), UAVs that keep the
// target they came with (fixed) and a limit on the UAVs of one target (capacity). The rule is in
// include/uavhip.h. Built with -ffp-contract=off: the tests compare assignments bit for bit with a
// Python restatement of the rule, and without constraints with k_search.
//
// One wave per row, four per workgroup, k_search's shape and its five instantiations. The row is
// RefineRow<.., LIM = true> (refine_device.hpp) and the scan is best_exchange (search_device.hpp), both
// k_search's own code; what LIM adds to the registers (RowLimits):
//   lane t, per target slot: ok, a 64-bit mask over the UAVs (bit u = allowed[u][t]), built once from
//           N byte rows, each a coalesced load of M bytes; cap = capacity[t];
//   fixed:  a ballot of the lanes' fixed flags, wave-uniform.
// The sweep's candidate test is a bit test and cnt < cap on the counts build_q forms anyway; a fixed
// UAV is a uniform skip in the sweep and in the scan. This file holds the start of the rule: the two
// passes that drop what the constraints do not admit. No LDS, no atomics; the env is only read.
#include "search_device.hpp"

namespace uavhip {
namespace {

// RowLimits from the row's arrays (a NULL array constrains nothing), then the start of the rule on
// r.a: pass 1 counts the fixed UAVs on their targets and their conflicts, pass 2 visits the free
// ones in ascending u and drops a pair that is not allowed or whose target is full so far.
template <int TPL, int NR>
__device__ __forceinline__ void start_limits(RefineRow<TPL, NR, true>& r, int s, const uint8_t* __restrict__ allowed,
                                             const uint8_t* __restrict__ fixed, const int* __restrict__ capacity,
                                             int& dropped, int& conflicts) {
    const int N = r.N, M = r.M, lane = r.lane;
    int cnt[TPL];
#pragma unroll
    for (int j = 0; j < TPL; ++j) {
        const int t = lane + kWave * j;
        unsigned long long ok = ~0ull;
        if (allowed) {
            ok = 0;
            const uint8_t* row = allowed + (long long)s * N * M;
            for (int u = 0; u < N; ++u)
                if (t < M && row[u * M + t]) ok |= 1ull << u;
        }
        r.lim.ok[j] = ok;
        int cap = 0x7fffffff;
        if (capacity && t < M) cap = capacity[(long long)s * M + t];
        r.lim.cap[j] = cap < 0 ? 0 : cap;
        cnt[j] = 0;
    }
    r.lim.fixed = ballot(fixed && r.isu && fixed[(long long)s * N + lane]);

    dropped = 0;
    conflicts = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int u = 0; u < N; ++u) {
            if ((int)(r.lim.fixed >> u & 1) == pass) continue;  // pass 0: the fixed UAVs; pass 1: the free ones
            const int au = readlane_i(r.a, u);
            if (au < 0) continue;
            unsigned long long pair = 0, room = 0;  // nonzero: u may take au; au has room so far
#pragma unroll
            for (int j = 0; j < TPL; ++j) {
                const bool mine = lane + kWave * j == au;
                pair |= ballot(mine && (r.lim.ok[j] >> u & 1));
                room |= ballot(mine && cnt[j] < r.lim.cap[j]);
            }
            if (pass == 0) {
                conflicts += (pair == 0) + (room == 0);
            } else if (pair == 0 || room == 0) {
                if (lane == u) r.a = -1;
                ++dropped;
                continue;
            }
#pragma unroll
            for (int j = 0; j < TPL; ++j)
                if (lane + kWave * j == au) ++cnt[j];
        }
    }
}

template <int TPL, int NR>
__global__ __launch_bounds__(64 * kRefineWaves) void k_search_constrained(
    uavhip_env env, int stride, int S, int max_exchanges, int max_sweeps, const uint8_t* __restrict__ allowed,
    const uint8_t* __restrict__ fixed, const int* __restrict__ capacity, const int* ain, int* aout,
    double* __restrict__ J, int* __restrict__ covered, int* __restrict__ stats) {
    const int s = blockIdx.x * kRefineWaves + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (s >= S) return;
    RefineRow<TPL, NR, true> r;
    r.load(env, s, stride, lane);
    r.convert(ain, s);
    int dropped, conflicts;
    start_limits(r, s, allowed, fixed, capacity, dropped, conflicts);
    r.load_columns();
    int exchanges = 0, scan_clean = 0;
    for (;;) {
        r.phase(max_sweeps);
        if (max_exchanges == 0) break;
        double bd;
        int bi, bj;
        best_exchange(r, bd, bi, bj);
        if (!(bd > 0.0)) {
            scan_clean = 1;
            break;
        }
        if (exchanges == max_exchanges) break;
        const int ai = readlane_i(r.a, bi), aj = readlane_i(r.a, bj);
        if (lane == bi) r.a = aj;
        if (lane == bj) r.a = ai;
        ++exchanges;
    }

    r.finish(s, aout, J, covered);
    if (stats && lane < 8)
        stats[(long long)s * 8 + lane] = lane == 0   ? r.sweeps
                                         : lane == 1 ? r.moves
                                         : lane == 2 ? r.converged
                                         : lane == 3 ? r.invalid
                                         : lane == 4 ? exchanges
                                         : lane == 5 ? scan_clean
                                         : lane == 6 ? dropped
                                                     : conflicts;
}

}  // namespace
}  // namespace uavhip

extern "C" int uavhip_search_assignments_constrained(const uavhip_env* env, int32_t env_stride, int32_t S,
                                                     int32_t max_exchanges, int32_t max_sweeps, const uint8_t* allowed,
                                                     const uint8_t* fixed, const int32_t* capacity,
                                                     const int32_t* assignment_in, int32_t* assignment_out, double* J,
                                                     int32_t* covered, int32_t* stats, uavhip_stream_t stream) {
    using namespace uavhip;
    if (const int rc = check_rows("uavhip_search_assignments_constrained", env, env_stride, S,
                                  max_exchanges >= 0 && max_sweeps >= 0 && assignment_out && J && covered,
                                  "max_exchanges=%d >= 0, max_sweeps=%d >= 0", max_exchanges, max_sweeps))
        return rc;
    UAVHIP_ROWS_LAUNCH(env, S, (k_search_constrained<TPL, NCAP>), stream, *env, (int)env_stride, (int)S, (int)max_exchanges,
                       (int)max_sweeps, allowed, fixed, capacity, assignment_in, assignment_out, J, covered, stats);
    return check_launch("k_search_constrained");
}
