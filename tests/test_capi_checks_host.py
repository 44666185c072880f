"""The argument checks of the C entry points and of their Python wrappers, pinned (no GPU): the
return code and the FULL text of uavhip_last_error() of every documented misuse, and the ValueError
texts of the wrappers' own checks. Every C case is refused on the host before any HIP call -- the
descriptors hold placeholder pointers that would fault if a kernel ran. The texts are literals: a
change of the layer between a caller and a launch that alters one of them shows up here."""
import ctypes

import pytest
import torch

from capi_host import _env_desc

P = ctypes.c_void_p(16)
u64 = ctypes.c_uint64
EINVAL = -1
NULL_ENV = "env descriptor is NULL"
DIMS = "bad env dims E=6 N={N} M={M} Kn=1 Ki=1 (N<=64, M<=128, Kn,Ki<=8)"
N65, M129 = DIMS.format(N=65, M=4), DIMS.format(N=8, M=129)


def _lib():
    from uavhip import _lib
    return _lib


def _policy_desc(n_floats=None):
    from uavhip.policy import split_layout
    p = _lib().PolicyDesc()
    p.weights = 16  # placeholder, never dereferenced by the checks
    p.n_floats = split_layout()[1] if n_floats is None else n_floats
    p.d_model, p.n_heads, p.d_ff, p.d_head_hidden, p.actor_layers, p.critic_layers = 128, 8, 256, 64, 1, 2
    return p


def packed_floats():
    from uavhip.policy import split_layout
    return split_layout()[1]


def ring_overflow_B():
    """The smallest B with B * 5 * kRowFloats >= 2^31 (the ring's offsets are 32-bit)."""
    f = _lib().LIB.uavhip_policy_rowproj_floats
    row = (f(2) - f(1)) // 5
    assert (f(2) - f(1)) % 5 == 0 and row > 0
    B = -(-2 ** 31 // (5 * row))
    assert B * 5 * row >= 2 ** 31 > (B - 1) * 5 * row
    return B


def refused(rc, text):
    got = _lib().LIB.uavhip_last_error().decode()
    assert rc == EINVAL and got == text, (rc, got)


def pos(args, **kw):
    """args: [(name, default)] in the entry point's order -> the positional list with kw applied."""
    assert set(kw) <= {n for n, _ in args}, kw
    return [kw.get(n, d) for n, d in args]


# ------------------------------------------------------------------ env-shaped entry points
def test_teacher_steps():
    fn, nm = _lib().LIB.uavhip_teacher_steps, "uavhip_teacher_steps: "
    args = [("env", None), ("asg", P), ("n_max", 4)] + [(k, P) for k in ("obs", "act", "rew", "done", "info", "steps",
                                                                          "fin", "ret", "stats")] + [("stream", None)]

    def call(**kw):
        a = pos(args, **kw)
        a[0] = a[0] if "env" in kw else _env_desc()
        return fn(*a)

    need = nm + "need n_max={} >= 1 and assignment/steps/finished non-NULL"
    refused(call(env=None), nm + NULL_ENV)
    refused(call(env=_env_desc(N=65)), nm + N65)
    refused(call(env=_env_desc(M=129)), nm + M129)
    refused(call(env=_env_desc(flags=_lib().ENV_OBS_F16)),
            nm + "f32 observations only (the env has UAVHIP_ENV_OBS_F16 set)")
    for k in ("asg", "steps", "fin"):
        refused(call(**{k: None}), need.format(4))
    refused(call(n_max=0), need.format(0))
    refused(call(n_max=-3), need.format(-3))


def test_expert_steps():
    fn, nm = _lib().LIB.uavhip_expert_steps, "uavhip_expert_steps: "
    args = [("env", None), ("act_in", P), ("follow", P), ("n_max", 4)] + \
           [(k, P) for k in ("obs", "act", "lab", "margin", "rew", "done", "steps", "fin", "ret", "stats")] + \
           [("stream", None)]

    def call(**kw):
        a = pos(args, **kw)
        a[0] = a[0] if "env" in kw else _env_desc()
        return fn(*a)

    need = nm + "need n_max={} >= 1 and steps/finished non-NULL"
    refused(call(env=None), nm + NULL_ENV)
    refused(call(env=_env_desc(N=65)), nm + N65)
    refused(call(env=_env_desc(M=129)), nm + M129)
    refused(call(env=_env_desc(flags=_lib().ENV_OBS_F16)),
            nm + "f32 observations only (the env has UAVHIP_ENV_OBS_F16 set)")
    refused(call(steps=None), need.format(4))
    refused(call(fin=None), need.format(4))
    refused(call(n_max=0), need.format(0))
    refused(call(act_in=None), nm + "follow needs actions_in (without a trace every env follows the expert)")


def test_refine_assignments():
    fn, nm = _lib().LIB.uavhip_refine_assignments, "uavhip_refine_assignments: "
    args = [("env", None), ("stride", 1), ("S", 6), ("sweeps", 4), ("ain", P), ("out", P), ("J", P), ("cov", P),
            ("stats", P), ("stream", None)]

    def call(**kw):
        a = pos(args, **kw)
        a[0] = a[0] if "env" in kw else _env_desc()
        return fn(*a)

    need = nm + ("need env_stride={} >= 1, S={} >= 1, (S - 1) * env_stride < E=6, max_sweeps={} >= 0 and "
                 "assignment_out/J/covered non-NULL")
    refused(call(env=None), nm + NULL_ENV)
    refused(call(env=_env_desc(N=65)), nm + N65)
    refused(call(env=_env_desc(M=129)), nm + M129)
    for k in ("out", "J", "cov"):
        refused(call(**{k: None}), need.format(1, 6, 4))
    refused(call(stride=0), need.format(0, 6, 4))
    refused(call(S=0), need.format(1, 0, 4))
    refused(call(S=7), need.format(1, 7, 4))
    refused(call(stride=2, S=4), need.format(2, 4, 4))
    refused(call(sweeps=-1), need.format(1, 6, -1))


def test_search_assignments():
    fn, nm = _lib().LIB.uavhip_search_assignments, "uavhip_search_assignments: "
    args = [("env", None), ("stride", 1), ("S", 6), ("exchanges", 3), ("sweeps", 4), ("ain", P), ("out", P), ("J", P),
            ("cov", P), ("stats", P), ("stream", None)]

    def call(**kw):
        a = pos(args, **kw)
        a[0] = a[0] if "env" in kw else _env_desc()
        return fn(*a)

    need = nm + ("need env_stride={} >= 1, S={} >= 1, (S - 1) * env_stride < E=6, max_exchanges={} >= 0, "
                 "max_sweeps={} >= 0 and assignment_out/J/covered non-NULL")
    refused(call(env=None), nm + NULL_ENV)
    refused(call(env=_env_desc(N=65)), nm + N65)
    refused(call(env=_env_desc(M=129)), nm + M129)
    for k in ("out", "J", "cov"):
        refused(call(**{k: None}), need.format(1, 6, 3, 4))
    refused(call(stride=0), need.format(0, 6, 3, 4))
    refused(call(S=0), need.format(1, 0, 3, 4))
    refused(call(S=7), need.format(1, 7, 3, 4))
    refused(call(stride=2, S=4), need.format(2, 4, 3, 4))
    refused(call(sweeps=-1), need.format(1, 6, 3, -1))
    refused(call(exchanges=-1), need.format(1, 6, -1, 4))


def test_select_best():
    fn = _lib().LIB.uavhip_select_best
    need = "uavhip_select_best: K={} must be > 0 and divide E=6, and best/J/covered/assignment non-NULL"
    refused(fn(None, 3, P, P, P, P, None), NULL_ENV)  # the env's own message, without the name
    refused(fn(_env_desc(N=65), 3, P, P, P, P, None), N65)
    refused(fn(_env_desc(M=129), 3, P, P, P, P, None), M129)
    for K in (0, -2, 4):
        refused(fn(_env_desc(), K, P, P, P, P, None), need.format(K))
    for i in range(4):
        out = [P] * 4
        out[i] = None
        refused(fn(_env_desc(), 3, *out, None), need.format(3))


# ------------------------------------------------------------------ the fused step entry points
# (policy, env, ...): the env's own message comes without the name; then the policy, the entry
# point's own condition, the ring
def step_cases(fn, name, args, cond, nulls, counts, f16):
    """The cases every step entry point shares. args: [(name, default)] with "pol", "env", "states",
    "rowproj", "step"; cond: the text of the entry point's own condition with {N} {M} and one {} per
    name in counts; nulls: its required outputs; counts: {argument: (ok value, bad values)}."""
    nm = name + ": "

    def call(**kw):
        a = pos(args, **kw)
        a[0] = a[0] if "pol" in kw else _policy_desc()
        a[1] = a[1] if "env" in kw else _env_desc()
        return fn(*a)

    def own(N=8, M=4, **kw):
        vals = [kw.get(k, ok) for k, (ok, _) in counts.items()]
        return nm + cond.format(*vals, N=N, M=M)

    ring = nm + "NULL rowproj, step={} < 0 or E={} above the ring's 32-bit offsets"
    refused(call(env=None), NULL_ENV)
    refused(call(env=_env_desc(N=65)), N65)
    refused(call(env=_env_desc(M=129)), M129)
    refused(call(env=_env_desc(M=65)), own(M=65))  # inside the ABI's M <= 128, beyond one env per wave
    if f16:
        refused(call(env=_env_desc(flags=_lib().ENV_OBS_F16)), own())
    for k in nulls:
        refused(call(**{k: None}), own())
    for k, (_, bad) in counts.items():
        for v in bad:
            refused(call(**{k: v}), own(**{k: v}))
    refused(call(step=-1), ring.format(-1, 6))
    refused(call(rowproj=None), ring.format(0, 6))
    big = ring_overflow_B()
    refused(call(env=_env_desc(E=big)), ring.format(0, big))
    refused(call(states=None), nm + "NULL policy/weights/states or B=6")
    refused(call(pol=_lib().PolicyDesc()), nm + "NULL policy/weights/states or B=6")
    n = packed_floats()
    for off in (n - 1, n + 1):
        refused(call(pol=_policy_desc(off)), nm + f"unsupported architecture / packed size {off} (expected {n})")


def test_rollout_step():
    args = [("pol", None), ("env", None), ("states", P), ("rowproj", P), ("step", 0), ("fill", 1), ("seed", u64(0)),
            ("offset", u64(0)), ("offset_dev", None), ("action", P), ("logp", P), ("value", P), ("auto_reset", 1),
            ("obs", P), ("reward", P), ("done", P), ("info", P), ("stream", None)]
    step_cases(_lib().LIB.uavhip_rollout_step, "uavhip_rollout_step", args,
               "N={N}, M={M} must be <= 64 and action/obs/reward/done non-NULL", ("action", "obs", "reward", "done"),
               {}, f16=False)


def test_rollout_steps():
    args = [("pol", None), ("env", None), ("states", P), ("rowproj", P), ("step", 0), ("n", 4), ("fill", 1),
            ("seed", u64(0)), ("offset", u64(0)), ("offset_stride", u64(0)), ("offset_dev", None), ("actions", P),
            ("logp", P), ("value", P), ("auto_reset", 1), ("reward", P), ("done", P), ("info", P), ("stream", None)]
    step_cases(_lib().LIB.uavhip_rollout_steps, "uavhip_rollout_steps", args,
               "N={N}, M={M} must be <= 64, observations f32, n={} > 0 and actions/logp/value/reward/done non-NULL",
               ("actions", "logp", "value", "reward", "done"), {"n": (4, (0, -2))}, f16=True)


def test_rollout_actor_steps():
    args = [("pol", None), ("env", None), ("states", P), ("rowproj", P), ("step", 0), ("n", 4), ("fill", 1),
            ("seed", u64(0)), ("offset", u64(0)), ("offset_stride", u64(0)), ("offset_dev", None), ("actions", P),
            ("logp", P), ("auto_reset", 1), ("reward", P), ("done", P), ("info", P), ("stream", None)]
    step_cases(_lib().LIB.uavhip_rollout_actor_steps, "uavhip_rollout_actor_steps", args,
               "N={N}, M={M} must be <= 64, observations f32, n={} > 0 and actions/logp/reward/done non-NULL",
               ("actions", "logp", "reward", "done"), {"n": (4, (0, -2))}, f16=True)


def test_decode_steps():
    args = [("pol", None), ("env", None), ("states", P), ("rowproj", P), ("step", 0), ("n_max", 4), ("fill", 1),
            ("greedy", 1), ("seed", u64(0)), ("offset", u64(0)), ("offset_stride", u64(0)), ("offset_dev", None),
            ("actions", None), ("steps", P), ("finished", P), ("ep_return", None), ("stream", None)]
    step_cases(_lib().LIB.uavhip_decode_steps, "uavhip_decode_steps", args,
               "N={N}, M={M} must be <= 64, observations f32, n_max={} > 0, greedy_stride={} >= 0 and "
               "steps/finished non-NULL", ("steps", "finished"), {"n_max": (4, (0, -3)), "greedy": (1, (-1,))},
               f16=True)


# ------------------------------------------------------------------ the ring entry points without an env
def policy_cases(call, nm, B):
    refused(call(states=None), nm + f"NULL policy/weights/states or B={B}")
    refused(call(pol=_lib().PolicyDesc()), nm + f"NULL policy/weights/states or B={B}")
    refused(call(B=0), nm + "NULL policy/weights/states or B=0")
    n = packed_floats()
    for off in (n - 1, n + 1):
        refused(call(pol=_policy_desc(off)), nm + f"unsupported architecture / packed size {off} (expected {n})")


def test_policy_forward_rows():
    fn, nm = _lib().LIB.uavhip_policy_forward_rows, "uavhip_policy_forward_rows: "
    args = [("pol", None), ("states", P), ("B", 6), ("rowproj", P), ("step", 0), ("fill", 1), ("actions_in", None),
            ("seed", u64(0)), ("offset", u64(0)), ("offset_dev", None), ("action", P), ("logp", P), ("value", P),
            ("entropy", None), ("logits", None), ("stream", None)]

    def call(**kw):
        a = pos(args, **kw)
        a[0] = a[0] if "pol" in kw else _policy_desc()
        return fn(*a)

    ring = nm + "NULL rowproj, step={} < 0 or B={} above the ring's 32-bit offsets"
    policy_cases(call, nm, 6)
    refused(call(step=-1), ring.format(-1, 6))
    refused(call(rowproj=None), ring.format(0, 6))
    big = ring_overflow_B()
    refused(call(B=big), ring.format(0, big))


def test_policy_value_rows():
    fn, nm = _lib().LIB.uavhip_policy_value_rows, "uavhip_policy_value_rows: "
    args = [("pol", None), ("states", P), ("B", 6), ("rowproj", P), ("step", 0), ("fill", 1), ("value", P),
            ("stream", None)]

    def call(**kw):
        a = pos(args, **kw)
        a[0] = a[0] if "pol" in kw else _policy_desc()
        return fn(*a)

    ring = nm + "NULL rowproj / value, step={} < 0 or B={} above the ring's 32-bit offsets"
    policy_cases(call, nm, 6)
    refused(call(step=-1), ring.format(-1, 6))
    refused(call(rowproj=None), ring.format(0, 6))
    refused(call(value=None), ring.format(0, 6))
    big = ring_overflow_B()
    refused(call(B=big), ring.format(0, big))


def test_value_steps():
    fn, nm = _lib().LIB.uavhip_value_steps, "uavhip_value_steps: "
    args = [("pol", None), ("states", P), ("B", 6), ("n", 4), ("rowproj", P), ("step", 0), ("fill", 1), ("values", P),
            ("last_values", None), ("stash", P), ("stream", None)]

    def call(**kw):
        a = pos(args, **kw)
        a[0] = a[0] if "pol" in kw else _policy_desc()
        return fn(*a)

    ring = nm + "NULL rowproj / values / stash, n={} <= 0, step={} < 0 or B={} above the ring's 32-bit offsets"
    policy_cases(call, nm, 6)
    refused(call(step=-1), ring.format(4, -1, 6))
    for k in ("rowproj", "values", "stash"):
        refused(call(**{k: None}), ring.format(4, 0, 6))
    refused(call(n=0), ring.format(0, 0, 6))
    refused(call(n=-2), ring.format(-2, 0, 6))
    big = ring_overflow_B()
    refused(call(B=big), ring.format(4, 0, big))


# ------------------------------------------------------------------ the Python wrappers' own checks
CPU = torch.device("cpu")


def _bare_env(E=6, N=8, M=4):
    """A VecUAVEnv without device state: what the wrappers' argument checks read."""
    from uavhip.vec_env import VecUAVEnv
    env = object.__new__(VecUAVEnv)
    env.E, env.N, env.M, env.device, env.obs_dtype = E, N, M, CPU, torch.float32
    return env


@pytest.mark.parametrize("fn", ["refine_assignments", "search_assignments"])
def test_rows_arguments_through_the_wrappers(fn):
    call = getattr(_bare_env(), fn)
    for kw, text in ((dict(stride=0), "stride=0 must be >= 1"), (dict(stride=-2), "stride=-2 must be >= 1"),
                     (dict(rows=7), "rows=7 at stride=1 do not fit E=6"),
                     (dict(rows=0), "rows=0 at stride=1 do not fit E=6"),
                     (dict(stride=2, rows=4), "rows=4 at stride=2 do not fit E=6"),
                     (dict(max_sweeps=-1), "max_sweeps=-1 must be >= 0")):
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert str(e.value) == f"{fn}: {text}"
    if fn == "search_assignments":
        with pytest.raises(ValueError) as e:
            call(max_exchanges=-1)
        assert str(e.value) == "search_assignments: max_exchanges=-1 must be >= 0"
    # a given buffer of the wrong layout is refused before the call, by name
    with pytest.raises(ValueError) as e:
        call(out=torch.zeros(8, 6, dtype=torch.int32).t())
    assert str(e.value) == ("out: need a contiguous torch.int32 tensor of 48 elements on cpu (got torch.int32 (6, 8) "
                            "on cpu, contiguous=False)")
    with pytest.raises(ValueError) as e:
        call(J=torch.zeros(6, dtype=torch.float32))
    assert str(e.value) == ("J: need a contiguous torch.float64 tensor of 6 elements on cpu (got torch.float32 (6,) "
                            "on cpu, contiguous=True)")


def test_check_out_texts():
    from uavhip.vec_env import check_out
    check_out(None, "mask", torch.uint8, (6,), CPU)
    check_out(torch.zeros(2, 3, 2, dtype=torch.uint8), "x", torch.uint8, (2, 3), CPU, (2,))
    for t, got in ((torch.zeros(5, dtype=torch.uint8), "torch.uint8 (5,) on cpu, contiguous=True"),
                   (torch.zeros(6, dtype=torch.int8), "torch.int8 (6,) on cpu, contiguous=True"),
                   (torch.zeros(12, dtype=torch.uint8)[::2], "torch.uint8 (6,) on cpu, contiguous=False"),
                   ([0] * 6, "list")):
        with pytest.raises(ValueError) as e:
            check_out(t, "mask", torch.uint8, (6,), CPU)
        assert str(e.value) == f"mask: need a contiguous torch.uint8 tensor of 6 elements on cpu (got {got})"
    with pytest.raises(ValueError) as e:
        check_out(torch.zeros(3, 6, dtype=torch.int8), "actions", torch.int8, (4, 6), CPU)
    assert str(e.value).startswith("actions: need a contiguous torch.int8 tensor of 24 elements on cpu")


def test_ring_check_through_the_wrappers():
    """A ring that is too short, of another dtype or strided is refused before the call, under the
    wrapper's name for the window count."""
    from uavhip.policy import TransformerActorCritic
    need = _lib().LIB.uavhip_policy_rowproj_floats(6)
    net = TransformerActorCritic()
    obs, values = torch.zeros(3, 6, 5, 14), torch.zeros(2, 6)
    steps, finished = torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.uint8)
    for bad in (torch.zeros(need - 1), torch.zeros(need, dtype=torch.float64), torch.zeros(2 * need)[::2]):
        with pytest.raises(ValueError) as e:
            net.value_steps(obs, bad, 0, values)
        assert str(e.value) == "rowproj: need a contiguous float32 rowproj_buffer(B)"
        with pytest.raises(ValueError) as e:
            net.decode_steps(_bare_env(), obs[:2], bad, 0, True, steps, finished, n_max=4)
        assert str(e.value) == "rowproj: need a contiguous float32 rowproj_buffer(E)"
