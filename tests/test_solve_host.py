"""Host-side checks of the inference entry points (no GPU): the argument checks of
uavhip_decode_steps / uavhip_select_best, AllocationSolver's refusal of a CPU policy, and the numpy
restatement of uavhip_select_best that tests/test_gpu_solve.py compares the kernel against."""
import ctypes

import numpy as np
import pytest
import torch

from capi_host import _env_desc


def select_best_np(uav_idx, J, covered, assigned, tgt_id, N, K):
    """uavhip_select_best restated (include/uavhip.h): envs e = s * K + k; per scene the FINISHED
    replica (uav_idx >= N) with the largest J, the lowest k on a tie. uav_idx / J / covered [E],
    assigned [E, N] (target list index or -1), tgt_id [E, M] of each env's active scene.
    -> best [S] (-1: none finished), J [S], covered [S], assignment [S, N] (target ids, -1 none)."""
    E = len(uav_idx)
    S = E // K
    best = np.full(S, -1, np.int32)
    Jb = np.zeros(S, np.float64)
    cov = np.zeros(S, np.int32)
    asg = np.full((S, N), -1, np.int32)
    for s in range(S):
        for k in range(K):
            e = s * K + k
            if uav_idx[e] < N:
                continue
            if best[s] < 0 or J[e] > Jb[s]:
                best[s], Jb[s] = k, J[e]
        if best[s] >= 0:
            e = s * K + best[s]
            cov[s] = covered[e]
            for u in range(N):
                if assigned[e, u] >= 0:
                    asg[s, u] = tgt_id[e, assigned[e, u]]
    return best, Jb, cov, asg


def test_select_best_restatement():
    N, K = 3, 4
    #            scene 0: replica 2 wins        scene 1: tie 1 = 3 -> 1      scene 2: none finished
    uav_idx = np.array([3, 3, 3, 1,             0, 3, 2, 3,                  0, 1, 2, 2])
    J = np.array([1.0, 2.0, 5.0, 9.0,           9.0, 4.0, 8.0, 4.0,          7.0, 7.0, 7.0, 7.0])
    covered = np.arange(12, dtype=np.int32)
    assigned = np.tile(np.array([1, -1, 0], np.int32), (12, 1))
    tgt_id = np.tile(np.array([7, 5], np.int32), (12, 1))
    tgt_id[5] = (2, 3)
    best, Jb, cov, asg = select_best_np(uav_idx, J, covered, assigned, tgt_id, N, K)
    assert best.tolist() == [2, 1, -1]          # arg-max J over finished; lowest replica on a tie; none
    assert Jb.tolist() == [5.0, 4.0, 0.0]       # the unfinished J = 9 / 8 replicas do not count
    assert cov.tolist() == [2, 5, 0]
    assert asg.tolist() == [[5, -1, 7], [3, -1, 2], [-1, -1, -1]]
    # a finished replica with a negative J still beats "none"
    b, j, _, _ = select_best_np(np.array([3, 0]), np.array([-2.0, 5.0]), covered[:2], assigned[:2], tgt_id[:2], N, 2)
    assert b.tolist() == [0] and j.tolist() == [-2.0]


def _policy_desc():
    from uavhip import _lib
    from uavhip.policy import split_layout
    p = _lib.PolicyDesc()
    p.weights = 16  # placeholder, never dereferenced by the checks
    p.n_floats = split_layout()[1]
    p.d_model, p.n_heads, p.d_ff, p.d_head_hidden, p.actor_layers, p.critic_layers = 128, 8, 256, 64, 1, 2
    return p


def test_decode_steps_argument_checks_without_gpu():
    """Every documented misuse of uavhip_decode_steps returns UAVHIP_EINVAL with a message, before
    any HIP call (the placeholders would fault if a kernel ran)."""
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_decode_steps, _lib.LIB.uavhip_last_error
    u64 = ctypes.c_uint64
    P = ctypes.c_void_p(16)

    def call(env, pol=None, obs2=P, rowproj=P, step=0, n_max=4, greedy=1, steps=P, finished=P):
        return fn(pol or _policy_desc(), env, obs2, rowproj, step, n_max, 1, greedy, u64(0), u64(0), u64(0), None,
                  None, steps, finished, None, None)

    assert call(_env_desc(N=100)) == -1 and b"bad env dims" in err()            # beyond the ABI's N
    assert call(_env_desc(M=100)) == -1 and b"uavhip_decode_steps" in err() and b"<= 64" in err()  # ABI: M <= 128
    assert call(_env_desc(flags=_lib.ENV_OBS_F16)) == -1 and b"observations f32" in err()
    assert call(_env_desc(), n_max=0) == -1 and b"n_max=0" in err()
    assert call(_env_desc(), n_max=-3) == -1 and b"n_max=-3" in err()
    assert call(_env_desc(), greedy=-1) == -1 and b"greedy_stride=-1" in err()
    assert call(_env_desc(), obs2=None) == -1 and b"uavhip_decode_steps" in err()
    assert call(_env_desc(), rowproj=None) == -1 and b"NULL rowproj" in err()
    assert call(_env_desc(), steps=None) == -1 and b"steps/finished" in err()
    assert call(_env_desc(), finished=None) == -1 and b"steps/finished" in err()
    assert call(_env_desc(), step=-1) == -1 and b"step=-1" in err()
    # the ring's 32-bit offsets: E * 5 * row floats must stay below 2^31
    row = (int(_lib.LIB.uavhip_policy_rowproj_floats(2)) - int(_lib.LIB.uavhip_policy_rowproj_floats(1))) // 5
    big = (1 << 31) // (5 * row) + 1
    assert call(_env_desc(E=big)) == -1 and b"32-bit offsets" in err()
    assert call(_env_desc(), pol=_lib.PolicyDesc()) == -1 and b"uavhip_decode_steps" in err()  # NULL weights


def test_select_best_argument_checks_without_gpu():
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_select_best, _lib.LIB.uavhip_last_error
    P = ctypes.c_void_p(16)
    assert fn(_env_desc(N=100), 1, P, P, P, P, None) == -1 and b"bad env dims" in err()
    assert fn(_env_desc(E=6), 0, P, P, P, P, None) == -1 and b"K=0" in err()
    assert fn(_env_desc(E=6), -2, P, P, P, P, None) == -1 and b"K=-2" in err()
    assert fn(_env_desc(E=6), 4, P, P, P, P, None) == -1 and b"divide E=6" in err()
    for i in range(4):
        args = [P, P, P, P]
        args[i] = None
        assert fn(_env_desc(E=6), 3, *args, None) == -1 and b"non-NULL" in err()


def test_solver_refuses_cpu_policy():
    """No CPU fallback: the solver raises on a policy that is not on a HIP device."""
    from uavhip import AllocationSolver
    from uavhip.policy import TransformerActorCritic
    with pytest.raises(RuntimeError, match="GPU"):
        AllocationSolver(TransformerActorCritic(), 4, 4)


def test_solver_argument_checks():
    from uavhip import AllocationSolver

    class OnGpu(torch.nn.Module):  # stands in for a device policy: only the device is looked at here
        def parameters(self, recurse=True):
            class P:
                device = torch.device("cuda", 0)
            return iter([P()])

    with pytest.raises(ValueError, match="<= 64"):
        AllocationSolver(OnGpu(), 65, 4)
    with pytest.raises(ValueError, match="samples"):
        AllocationSolver(OnGpu(), 4, 4, samples=0)
    s = AllocationSolver(OnGpu(), 4, 4, samples=2)
    with pytest.raises(ValueError, match="scenes or num_scenes"):
        s.solve()
    with pytest.raises(ValueError, match="scenes or num_scenes"):
        s.solve(scenes=[{}], num_scenes=1)


def test_decode_steps_code_object(tmp_path):
    """tests/test_codeobject.py's limits on k_decode_steps (both env-path instantiations), and one env
    path only per instantiation: the grouped one is the smaller."""
    import os
    import subprocess
    import test_codeobject as tc
    if not os.path.exists(tc.HIPCC) or not os.path.exists(tc.READELF):
        pytest.skip("needs hipcc and llvm-readelf")
    asm = tc.compile_asm("rollout_steps.hip", tmp_path)
    ks = {k: v for k, v in tc.kernels(asm).items() if "k_decode_steps" in k}
    assert len(ks) == 2, list(ks)
    for name, m in ks.items():
        tc.check_limits(name, m)
    out = tmp_path / "rs.o"
    subprocess.run([tc.HIPCC] + [f for f in tc.FLAGS if f != "-S"] + ["--no-gpu-bundle-output", "-c",
                   tc.os.path.join(tc.CSRC, "rollout_steps.hip"), "-o", str(out)], check=True, cwd=tc.CSRC,
                   capture_output=True, timeout=600)
    syms = subprocess.run([tc.READELF, "-sW", str(out)], check=True, capture_output=True, text=True).stdout
    sizes = {l.split()[7]: int(l.split()[2]) for l in syms.splitlines() if " FUNC " in l and "k_decode_steps" in l}
    print(sizes)
    grp = next(v for k, v in sizes.items() if "k_decode_stepsILi1E" in k)
    wave = next(v for k, v in sizes.items() if "k_decode_stepsILi2E" in k)
    # with both env paths in one kernel the rollout's grew from 58.5 to 71 KB (test_codeobject.py); the
    # decode kernels carry the actor trunk only: 23 / 26 KB today
    assert grp <= 28 * 1024 and wave <= 31 * 1024, sizes
