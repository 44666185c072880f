// refine.hip -- best-response local search on the objective J(X) itself (uavhip_refine_assignments):
// polish a decoded allocation, build a non-learned baseline from the empty one, or only score an
// assignment that did not come from the env. The env decides each assignment on r(X) in one pass of
// the pointer walk (uav_env.py:295-435) and never revisits a UAV; here every UAV in turn moves to the
// target (or to none) where its marginal contribution to J (_calc_J_X, uav_env.py:244-269), the
// others held fixed, is largest. Built with -ffp-contract=off: the tests compare assignments bit for
// bit with a numpy restatement of the rule (include/uavhip.h).
//
// One wave per scene, four per workgroup (as k_select_best); the wave's view of its row -- registers,
// id conversion, sweeps, scoring -- is RefineRow (refine_device.hpp), which k_search (search.hip)
// runs too. The env and the scene are only read.
#include "refine_device.hpp"

namespace uavhip {
namespace {

template <int TPL, int NCAP>
__global__ __launch_bounds__(64 * kRefineWaves) void k_refine(uavhip_env env, int stride, int S, int max_sweeps,
                                                              const int* ain, int* aout, double* __restrict__ J,
                                                              int* __restrict__ covered, int* __restrict__ stats) {
    const int s = blockIdx.x * kRefineWaves + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (s >= S) return;
    RefineRow<TPL, NCAP> r;
    r.load(env, s, stride, lane);
    r.convert(ain, s);
    r.load_columns();
    r.phase(max_sweeps);
    r.finish(s, aout, J, covered);
    if (stats && lane < 4)
        stats[(long long)s * 4 + lane] = lane == 0 ? r.sweeps : lane == 1 ? r.moves : lane == 2 ? r.converged : r.invalid;
}

}  // namespace
}  // namespace uavhip

extern "C" int uavhip_refine_assignments(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t max_sweeps,
                                         const int32_t* assignment_in, int32_t* assignment_out, double* J,
                                         int32_t* covered, int32_t* stats, uavhip_stream_t stream) {
    using namespace uavhip;
    if (const int rc = check_rows("uavhip_refine_assignments", env, env_stride, S,
                                  max_sweeps >= 0 && assignment_out && J && covered, "max_sweeps=%d >= 0", max_sweeps))
        return rc;
    UAVHIP_ROWS_LAUNCH(env, S, (k_refine<TPL, NCAP>), stream, *env, (int)env_stride, (int)S, (int)max_sweeps, assignment_in,
                       assignment_out, J, covered, stats);
    return check_launch("k_refine");
}
