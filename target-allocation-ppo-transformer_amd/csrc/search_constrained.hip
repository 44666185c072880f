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
// UAV is a uniform skip in the sweep and in the scan. The start of the rule (start_limits: the two
// passes that drop what the constraints do not admit) is in search_device.hpp and the loop of phases and
// exchanges in search_loop_body.hpp, where k_search_multistart shares them. No LDS, no atomics; the env
// is only read.
#include "search_device.hpp"

namespace uavhip {
namespace {

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
#include "search_loop_body.hpp"

    r.finish(s, aout, J, covered);
    if (stats && lane < 8)
        stats[(long long)s * 8 + lane] = search_stat(r, lane, exchanges, scan_clean, dropped, conflicts);
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
