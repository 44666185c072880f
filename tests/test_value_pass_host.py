"""Host-side argument checks of uavhip_rollout_actor_steps / uavhip_value_steps (no GPU): every misuse
returns UAVHIP_EINVAL with a message before any HIP call, as test_rollout_step_argument_checks_without_gpu
expects of uavhip_rollout_step."""
import ctypes

from capi_host import _env_desc


def test_rollout_actor_steps_argument_checks_without_gpu():
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_rollout_actor_steps, _lib.LIB.uavhip_last_error
    pol = _lib.PolicyDesc()
    args = (None, None, 0, 4, 1, ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), None, None, None, 1,
            None, None, None, None)
    d = _lib.EnvDesc()
    d.E, d.N, d.M, d.Kn, d.Ki, d.scene_buffers = 4, 100, 4, 1, 1, 1
    assert fn(pol, d, *args) == -1 and b"bad env dims" in err()
    assert fn(pol, _env_desc(), *args) == -1 and b"uavhip_rollout_actor_steps" in err()  # NULL weights / obs


def test_value_steps_argument_checks_without_gpu():
    from uavhip import _lib
    fn, err = _lib.LIB.uavhip_value_steps, _lib.LIB.uavhip_last_error
    pol = _lib.PolicyDesc()
    assert fn(pol, None, 4, 3, None, 0, 1, None, None, None, None) == -1 and b"uavhip_value_steps" in err()
    assert fn(pol, 16, 0, 3, 16, 0, 1, 16, None, 16, None) == -1 and b"uavhip_value_steps" in err()  # B = 0
    # a policy of the right architecture: the pass's own arguments are checked next
    pol.weights, pol.n_floats = 16, _lib.LIB.uavhip_policy_split_layout(None, None, 0)
    pol.d_model, pol.n_heads, pol.d_ff, pol.d_head_hidden, pol.actor_layers, pol.critic_layers = 128, 8, 256, 64, 1, 2
    for bad in (dict(n=0), dict(step=-1), dict(rowproj=None), dict(values=None), dict(stash=None)):
        a = dict(n=3, step=0, rowproj=16, values=16, stash=16)
        a.update(bad)
        rc = fn(pol, 16, 4, a["n"], a["rowproj"], a["step"], 0, a["values"], None, a["stash"], None)
        assert rc == -1 and b"uavhip_value_steps" in err(), bad
    assert _lib.LIB.uavhip_value_steps_stash_floats(0) == -1
    assert _lib.LIB.uavhip_value_steps_stash_floats(17) == 2 * 5 * 2 * 16 * 136
