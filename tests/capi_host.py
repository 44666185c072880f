"""Shared pieces of the host-side tests of the C entry points (no GPU): the module fixture that
requires an entry point in the library, and placeholder descriptors for argument checks that must
fail before any HIP call. A plain module, imported by the test files (as adam_model.py is)."""
import pytest


def _entry_point(name):
    """-> an autouse module fixture: everything in the module restates or calls entry point `name`,
    without it in the library it means nothing. Use as `_entry_point = capi_host._entry_point(name)`."""
    @pytest.fixture(autouse=True, scope="module")
    def fixture():
        from uavhip import _lib
        assert name in _lib.EXPORTS and hasattr(_lib.LIB, name)
    return fixture


def _env_desc(N=8, M=4, E=6, flags=0):
    from uavhip import _lib
    d = _lib.EnvDesc()
    d.E, d.N, d.M, d.Kn, d.Ki, d.scene_buffers, d.flags = E, N, M, 1, 1, 1, flags
    for name in ("uav_pos", "uav_vel", "uav_load", "uav_cost", "tgt_pos", "tgt_vel", "tgt_value", "tgt_id", "nfz_pos",
                 "icp_pos", "icp_vel", "p_dmg", "p_pen", "istate", "nh_final", "nh_pure", "t_cost", "n_lock",
                 "assigned", "dstate", "window"):
        setattr(d, name, 16)  # non-NULL placeholders: validation never dereferences them
    return d
