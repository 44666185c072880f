// search.hip -- exchange-move local search on J(X) (uavhip_search_assignments): the best-response
// sweeps of uavhip_refine_assignments, and, where no single move improves J any more, the best
// pairwise exchange -- UAVs i and j swap their targets, one of which may be "none" -- after which the
// sweeps run again; until neither neighbourhood improves J or max_exchanges exchanges are made. The
// rule is in include/uavhip.h. Built with -ffp-contract=off: the tests compare assignments bit for
// bit with a Python restatement of the rule.
//
// One wave per row, four per workgroup; the row's registers and the sweeps are RefineRow
// (refine_device.hpp), k_refine's own; the scan over the pairs is best_exchange
// (search_device.hpp), which k_search_constrained (search_constrained.hip) runs too, and the loop of
// phases and exchanges is search_loop_body.hpp, theirs as well. No LDS, no atomics, nothing shared
// between waves; the env and the scene are only read.
#include "search_device.hpp"

namespace uavhip {
namespace {

template <int TPL, int NR>
__global__ __launch_bounds__(64 * kRefineWaves) void k_search(uavhip_env env, int stride, int S, int max_exchanges,
                                                              int max_sweeps, const int* ain, int* aout,
                                                              double* __restrict__ J, int* __restrict__ covered,
                                                              int* __restrict__ stats) {
    const int s = blockIdx.x * kRefineWaves + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (s >= S) return;
    RefineRow<TPL, NR> r;
    r.load(env, s, stride, lane);
    r.convert(ain, s);
    r.load_columns();
#include "search_loop_body.hpp"

    r.finish(s, aout, J, covered);
    if (stats && lane < 6)
        stats[(long long)s * 6 + lane] = lane == 0   ? r.sweeps
                                         : lane == 1 ? r.moves
                                         : lane == 2 ? r.converged
                                         : lane == 3 ? r.invalid
                                         : lane == 4 ? exchanges
                                                     : scan_clean;
}

}  // namespace
}  // namespace uavhip

extern "C" int uavhip_search_assignments(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t max_exchanges,
                                         int32_t max_sweeps, const int32_t* assignment_in, int32_t* assignment_out,
                                         double* J, int32_t* covered, int32_t* stats, uavhip_stream_t stream) {
    using namespace uavhip;
    if (const int rc = check_rows("uavhip_search_assignments", env, env_stride, S,
                                  max_exchanges >= 0 && max_sweeps >= 0 && assignment_out && J && covered,
                                  "max_exchanges=%d >= 0, max_sweeps=%d >= 0", max_exchanges, max_sweeps))
        return rc;
    UAVHIP_ROWS_LAUNCH(env, S, (k_search<TPL, NCAP>), stream, *env, (int)env_stride, (int)S, (int)max_exchanges,
                       (int)max_sweeps, assignment_in, assignment_out, J, covered, stats);
    return check_launch("k_search");
}
