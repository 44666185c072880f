"""The helpers the Python wrappers share, called directly with CPU tensors (no GPU): check_out and
out_buf (uavhip/_lib.py), _check_ring (uavhip/policy.py) and _rows_args (uavhip/vec_env.py). The same
messages through the wrappers themselves: tests/test_capi_checks_host.py."""
import pytest
import torch

from test_capi_checks_host import CPU, _lib


def test_check_out_has_one_home():
    from uavhip import _lib, policy, vec_env
    assert vec_env.check_out is _lib.check_out and policy.check_out is _lib.check_out


def test_out_buf():
    from uavhip._lib import out_buf
    given = torch.ones(4, 6, dtype=torch.float64)
    assert out_buf(given, "reward", torch.float64, (4, 6), CPU) is given
    assert out_buf(given, "reward", torch.float64, (4,), CPU, (6,), zero=True) is given and bool((given == 1).all())
    with pytest.raises(ValueError) as e:
        out_buf(given, "reward", torch.float64, (4, 5), CPU)
    assert str(e.value) == ("reward: need a contiguous torch.float64 tensor of 20 elements on cpu (got torch.float64 "
                            "(4, 6) on cpu, contiguous=True)")
    with pytest.raises(ValueError, match="stats: need a contiguous torch.int32 tensor of 12 elements on cpu"):
        out_buf(given, "stats", torch.int32, (6,), CPU, (2,))
    fresh = out_buf(None, "obs", torch.float32, (3, 6), CPU, (5, 14))
    assert fresh.dtype == torch.float32 and fresh.shape == (3, 6, 5, 14) and fresh.device == CPU and \
        fresh.is_contiguous()
    for dtype in (torch.int32, torch.uint8, torch.float64):
        z = out_buf(None, "steps", dtype, (6,), CPU, zero=True)
        assert z.dtype == dtype and z.shape == (6,) and not bool(z.any())
    st = out_buf(None, "stats", torch.int32, (6,), CPU, (3,))
    assert st.dtype == torch.int32 and st.shape == (6, 3)


def test_check_ring():
    from uavhip.policy import _check_ring
    need = _lib().LIB.uavhip_policy_rowproj_floats(6)
    _check_ring(torch.zeros(need), 6, "E")
    _check_ring(torch.zeros(need + 3), 6, "B")
    for what in ("E", "B"):
        for bad in (torch.zeros(need - 1), torch.zeros(need, dtype=torch.float64), torch.zeros(2 * need)[::2]):
            with pytest.raises(ValueError) as e:
                _check_ring(bad, 6, what)
            assert str(e.value) == f"rowproj: need a contiguous float32 rowproj_buffer({what})"


def test_rows_args():
    from uavhip.vec_env import _rows_args
    assert _rows_args("refine_assignments", 6, 1, None, max_sweeps=4) == 6
    assert _rows_args("refine_assignments", 6, 4, None, max_sweeps=0) == 2
    assert _rows_args("search_assignments", 6, 2, 3, max_exchanges=0, max_sweeps=1) == 3
    for kw, text in ((dict(stride=0, rows=None), "stride=0 must be >= 1"),
                     (dict(stride=1, rows=7), "rows=7 at stride=1 do not fit E=6"),
                     (dict(stride=1, rows=None, max_sweeps=-1), "max_sweeps=-1 must be >= 0"),
                     (dict(stride=1, rows=None, max_exchanges=-1, max_sweeps=2), "max_exchanges=-1 must be >= 0")):
        with pytest.raises(ValueError) as e:
            _rows_args("f", 6, **kw)
        assert str(e.value) == "f: " + text
