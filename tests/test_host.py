"""CPU-only checks of the product's host side and of the C-ABI library (no GPU compute):
library loads and exports every symbol include/uavhip.h declares; ctypes mirrors match the
header; the host scene generator reproduces the reference's scenes; the policy module matches the
reference's initialisation and state_dict; the packed-weight layout covers every parameter."""
import os
import random
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, cases, sub

HEADER = os.path.join(ROOT, "include", "uavhip.h")


def _header_functions():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(uavhip_\w+)\s*\(", txt, re.M)))


def _header_enum(name):
    txt = open(HEADER).read()
    body = re.search(r"enum " + name + r" \{(.*?)\};", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out, val = {}, -1
    for item in [x.strip() for x in body.split(",") if x.strip()]:
        if "=" in item:
            k, v = [y.strip() for y in item.split("=")]
            val = int(v)
        else:
            k = item
            val += 1
        out[k] = val
    return out


def test_library_exports_every_header_symbol():
    from uavhip import _lib
    fns = _header_functions()
    assert len(fns) >= 12
    for f in fns:
        assert hasattr(_lib.LIB, f), f
    assert set(fns) == set(_lib.EXPORTS)
    assert _lib.LIB.uavhip_abi_version() == _lib.ABI_VERSION == 6


def test_ctypes_mirrors_header_enums():
    from uavhip import _lib
    for enum, table, prefix in [("uavhip_info", _lib.INFO, "UAVHIP_INFO_"), ("uavhip_ist", _lib.IST, "UAVHIP_IST_"),
                                ("uavhip_dst", _lib.DST, "UAVHIP_DST_"), ("uavhip_param", _lib.PRM, "UAVHIP_PRM_"),
                                ("uavhip_gen", _lib.GEN, "UAVHIP_GEN_")]:
        h = _header_enum(enum)
        for k, v in table.items():
            assert h[prefix + k] == v, (enum, k)
    assert _header_enum("uavhip_info")["UAVHIP_INFO_COUNT"] == _lib.INFO_COUNT
    assert _header_enum("uavhip_param")["UAVHIP_PRM_COUNT"] == _lib.PRM_COUNT
    # struct field order: pointer fields in the header's order
    txt = open(HEADER).read()
    body = re.search(r"typedef struct uavhip_env \{(.*?)\} uavhip_env;", txt, re.S).group(1)
    names = re.findall(r"\*\s*(\w+);", body)
    assert names == [f[0] for f in _lib.EnvDesc._fields_[12:]]
    scalars = re.findall(r"u?int\w*_t\s+(\w+);", body.split("double prm")[0])
    assert scalars[-2:] == ["seed", "env_base"] == [f[0] for f in _lib.EnvDesc._fields_[8:10]]
    assert _header_enum("uavhip_ist")["UAVHIP_IST_COUNT"] == _lib.IST_COUNT
    assert _header_enum("uavhip_dst")["UAVHIP_DST_COUNT"] == _lib.DST_COUNT
    ph = _header_enum("uavhip_ppo_phase")
    assert (ph["UAVHIP_PPO_FORWARD"], ph["UAVHIP_PPO_BACKWARD"], ph["UAVHIP_PPO_UPDATE"], ph["UAVHIP_PPO_FULL"],
            ph["UAVHIP_PPO_PACKED"]) == (_lib.PPO_FORWARD, _lib.PPO_BACKWARD, _lib.PPO_UPDATE, _lib.PPO_FULL,
                                         _lib.PPO_PACKED)
    fl = _header_enum("uavhip_ppo_flag")
    names = ("NO_POS_SPLIT", "NO_TRUNK_SPLIT", "WGRAD_STREAM_K", "FIXED_ORDER_FWD", "FIXED_ORDER_BWD",
             "NO_GRAD_PRESCALE")
    bits = [fl["UAVHIP_PPO_" + k] for k in names]
    assert bits == [getattr(_lib, "PPO_" + k) for k in names] == [1 << i for i in range(6)]
    assert fl["UAVHIP_PPO_FLAGS_ALL"] == sum(bits) and len(fl) == 7


def _struct_fields(name):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        out += [re.findall(r"\w+", part)[-1] for part in decl.replace("*", " ").split(",")]
    return out


def _struct_types(name):
    """[(field, C type)] of a header struct (pointers as 'ptr')."""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = decl.split()[0] if not decl.startswith("const") else decl.split()[1]
        for part in decl.split(","):
            nm = re.findall(r"\w+", part.replace("*", " "))[-1]
            out.append((nm, "ptr" if "*" in part or ("*" in decl and part is decl.split(",")[0]) else base))
    return out


def test_ctypes_mirrors_header_structs():
    import ctypes
    from uavhip import _lib
    assert _struct_fields("uavhip_ppo") == [f[0] for f in _lib.PPODesc._fields_]
    # and the field types: the Adam hyper-parameters are doubles (torch's Python floats)
    kinds = {"float": ctypes.c_float, "double": ctypes.c_double, "int32_t": ctypes.c_int32, "ptr": ctypes.c_void_p}
    for (nm, ty), (fn, ft) in zip(_struct_types("uavhip_ppo"), _lib.PPODesc._fields_):
        assert nm == fn and ft is kinds[ty], (nm, ty, ft)
    assert _struct_fields("uavhip_policy") == [f[0] for f in _lib.PolicyDesc._fields_]
    assert _lib.LIB.uavhip_ppo_workspace_floats(64) > 0
    assert _lib.LIB.uavhip_ppo_workspace_floats(4096) > _lib.LIB.uavhip_ppo_workspace_floats(64)
    assert _lib.LIB.uavhip_ppo_workspace_floats(65) == -1


def test_error_path_without_gpu():
    """A bad descriptor is rejected by argument validation with a message, before any HIP call."""
    from uavhip import _lib
    d = _lib.EnvDesc()
    d.E, d.N, d.M = 1, 100, 4
    rc = _lib.LIB.uavhip_score_pairs(d, None, None)
    assert rc == -1 and b"bad env dims" in _lib.LIB.uavhip_last_error()
    with pytest.raises(_lib.UavHipError):
        _lib.check(rc, "uavhip_score_pairs")


def test_ppo_step_rejects_undefined_flag_bits_without_gpu():
    """uavhip_ppo.flags: a bit outside the UAVHIP_PPO_* variant bits is UAVHIP_EINVAL with a message
    that names `flags`, before any HIP call. Every other field of the descriptor is valid (placeholder
    pointers: validation never dereferences them), so the flags are what is refused."""
    from uavhip import _lib
    d = _lib.PPODesc()
    for name in ("params", "grads", "adam_m", "adam_v", "adam_step", "workspace", "loss_sums", "stats"):
        setattr(d, name, 16)
    d.n_floats, d.minibatch, d.global_minibatch = _lib.LIB.uavhip_policy_layout(None, 0), 64, 64
    d.lr_actor, d.lr_critic, d.beta1, d.beta2, d.adam_eps = 2e-4, 1e-3, 0.9, 0.999, 1e-8
    d.eps_clip, d.max_grad_norm, d.value_coef, d.entropy_coef = 0.2, 1.0, 0.5, 0.01
    args = (16, 16, 16, 16, 16, 16, 16, _lib.PPO_FULL, None)
    for flags in (64, 63 | 1 << 20, -1):
        d.flags = flags
        assert _lib.LIB.uavhip_ppo_step(d, *args) == -1
        assert b"uavhip_ppo_step: flags" in _lib.LIB.uavhip_last_error()


def test_host_scene_generator_matches_reference(traj_npz):
    from uavhip.config import Config, config0_overrides
    from uavhip.scene import generate_scene
    for c in cases(traj_npz):
        s = sub(traj_npz, c["key"])
        cf = Config()
        if c["cfg"] == "0":
            for k, v in config0_overrides().items():
                setattr(cf, k, v)
        cf.NUM_UAVS, cf.NUM_TARGETS = c["N"], c["M"]
        np.random.seed(c["seed"]); random.seed(c["seed"])
        g = generate_scene(cf)
        for k in ("uav_pos", "uav_vel", "uav_load", "uav_cost", "uav_type", "tgt_pos", "tgt_vel", "tgt_value",
                  "tgt_id", "nfz_pos", "icp_pos", "icp_vel"):
            np.testing.assert_array_equal(g[k], s[k], err_msg=f"{c['key']} {k}")
        assert g["total_swarm_cost"] == float(s["total_swarm_cost"])


def test_policy_init_matches_reference(policy_npz):
    from uavhip.policy import TransformerActorCritic
    torch.manual_seed(0)
    net = TransformerActorCritic()
    sd = net.state_dict()
    assert sum(p.numel() for p in net.parameters()) == int(policy_npz["nparams"]) == 419267
    import json
    assert list(sd.keys()) == json.loads(str(policy_npz["keys"]))
    for k, v in sd.items():
        np.testing.assert_array_equal(v.numpy(), policy_npz["a/w/" + k], err_msg=k)


def test_construction_leaves_the_cpu_generator_where_the_reference_does():
    """tests/golden/init_rng.npz: the reference's first sampler permutation (ppo.py:115,
    torch.randperm) after building two networks (PPOAgent's policy + policy_old, ppo.py:13-43) under
    torch.manual_seed(s). The build's networks draw nothing beyond the reference's initialisation
    (the Philox sampling key comes from torch.initial_seed()), so the minibatch orders of every
    later update() are the reference's. Different instances still get different sampling keys."""
    from conftest import load_golden
    from uavhip.policy import TransformerActorCritic
    f = load_golden("init_rng.npz")
    for s in (0, 7):
        torch.manual_seed(s)
        a, b = TransformerActorCritic(), TransformerActorCritic()
        np.testing.assert_array_equal(torch.randperm(192).numpy(), f[f"two_nets/{s}"])
        np.testing.assert_array_equal(f[f"two_nets/{s}"], f[f"agent/{s}"])  # PPOAgent draws nothing else
        assert a.sample_seed != b.sample_seed and 0 <= a.sample_seed < 2 ** 62


def test_policy_torch_path_matches_reference(policy_npz):
    """evaluate() (torch path used by the PPO update) reproduces the reference outputs on CPU."""
    from uavhip.policy import TransformerActorCritic
    net = TransformerActorCritic()
    net.load_state_dict({k[4:]: torch.from_numpy(policy_npz[k].copy()) for k in policy_npz.files
                         if k.startswith("b/w/")})
    x = torch.from_numpy(policy_npz["states"])
    a = torch.from_numpy(policy_npz["actions"])
    with torch.no_grad():
        logp, v, ent = net.evaluate(x, a)
    np.testing.assert_allclose(logp.numpy(), policy_npz["b/logp"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(v.numpy()[:, 0], policy_npz["b/value"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ent.numpy(), policy_npz["b/entropy"], rtol=1e-5, atol=1e-6)


def test_packed_layout_covers_state_dict():
    from uavhip.policy import TransformerActorCritic, from_fragment_order, layout, pack_weights, tiling
    offs, n = layout()
    net = TransformerActorCritic()
    sd = net.state_dict()
    sizes = [v.numel() for v in sd.values()]
    ends = offs[1:] + [n]
    for (k, v), o, e in zip(sd.items(), offs, ends):
        assert o % 4 == 0 and e - o >= v.numel() and e - o - v.numel() < 4, k
    buf = pack_weights(sd)
    kcols = tiling()
    assert sum(1 for K in kcols if K) == 14  # in_proj, out_proj, linear1, linear2 x 3 layers + 2 head.0
    for (k, v), o, K in zip(sd.items(), offs, kcols):
        got = buf[o:o + v.numel()]
        if K:
            assert k.endswith("weight") and v.shape[1] == K, k
            assert torch.equal(from_fragment_order(got, v.shape[0], K), v), k
            # spot-check the documented index formula (include/uavhip.h)
            r, c = v.shape[0] - 3, K - 6
            idx = ((r // 16 * (K // 16) + c // 16) * 64 + r % 16 + 16 * ((c % 16) // 4)) * 4 + c % 4
            assert got[idx] == v[r, c], k
        else:
            assert torch.equal(got, v.reshape(-1)), k
    assert n == sum((s + 3) // 4 * 4 for s in sizes)


def test_split_copies_encode_the_weights():
    """The split copies after the 50 parameters (include/uavhip.h uavhip_policy_split_layout): two
    fp16 planes per weight, w1 = f16(w), w2 = f16((w - w1) * 2^11), in 16 x 32 blocks (1 KiB of w1,
    then 1 KiB of w2; lane = r%16 + 16 ((k%32)//8) holding k%8). w1 + 2^-11 w2 = w to 2^-22 relative."""
    from uavhip.policy import TransformerActorCritic, layout, pack_weights, split_layout
    _, n = layout()
    splits, total = split_layout()
    from uavhip.policy import RANGE_FLOATS
    assert splits and total == n + sum(list(TransformerActorCritic().state_dict().values())[q].numel()
                                       for q, _ in splits) + RANGE_FLOATS
    torch.manual_seed(3)
    sd = TransformerActorCritic().state_dict()
    buf = pack_weights(sd)
    assert buf.numel() == total
    items = list(sd.items())
    for q, o in splits:
        k, w = items[q]
        R, K = w.shape
        planes = buf[o:o + R * K].view(torch.float16).reshape(R // 16, K // 32, 2, 64, 8).float()
        for r, c in ((0, 0), (R - 3, K - 6), (17, 45)):
            lane, j = r % 16 + 16 * ((c % 32) // 8), c % 8
            w1, w2 = planes[r // 16, c // 32, 0, lane, j], planes[r // 16, c // 32, 1, lane, j]
            assert w1 == torch.tensor(float(w[r, c])).half().float(), k
            assert abs(float(w1 + w2 / 2048) - float(w[r, c])) <= 2 ** -22 * abs(float(w[r, c])) + 2 ** -35, k
        dec = planes[:, :, 0] + planes[:, :, 1] / 2048  # [R/16][K/32][64][8] -> [R][K]
        dec = dec.reshape(R // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(R, K)
        # 2^-22 relative; below fp16's normal range (|w| < 2^-14) w1 is subnormal and the bound is
        # 2^-24 * 2^-11 absolute
        assert bool(((dec - w).abs() <= 2 ** -22 * w.abs() + 2 ** -35).all()), k


def test_config_matches_reference_constants(traj_npz):
    from uavhip.config import cfg, params_vector
    s = sub(traj_npz, "c0")
    np.testing.assert_array_equal(params_vector(cfg), s["params"])
    assert (cfg.GAMMA, cfg.GAE_LAMBDA, cfg.K_EPOCHS, cfg.EPS_CLIP, cfg.BATCH_SIZE) == (0.998, 0.95, 5, 0.2, 64)


def test_product_refuses_cpu():
    """No silent CPU fallback: the product env and agent refuse to run without a GPU."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from uavhip.vec_env import VecUAVEnv
    from uavhip.ppo import PPOAgent
    from uavhip.policy import TransformerActorCritic
    with pytest.raises(RuntimeError):
        VecUAVEnv(4, 4, 4, device="cpu")
    with pytest.raises(RuntimeError):
        PPOAgent()
    with pytest.raises(RuntimeError):
        TransformerActorCritic().get_action(torch.zeros(1, 5, 14))


def test_csv_rows_follow_main_train_columns():
    """metrics.csv_rows: main_train.py:56-61 columns, :165-173 ratios (denominators clamped to 1)."""
    from uavhip import _lib
    from uavhip.metrics import CSV_HEADER, csv_rows
    E = _lib.EP
    rec = np.zeros((2, _lib.EP_COUNT))
    rec[0, [E["STEPS"], E["REWARD"], E["Q0"], E["J_SUM"], E["MAX_COV"], E["ACTION1"], E["VALID"]]] = [4, 2.0, 0.5, 8.0, 3, 2, 1]
    rec[0, [E["PDMG_SUM"], E["PFINAL_SUM"], E["ASSIGN_STEPS"]]] = [1.2, 0.6, 3]
    rec[1, [E["STEPS"], E["REWARD"], E["Q0"]]] = [1, 4.0, 1.5]          # no assigns, no action 1
    rows = csv_rows(rec, losses=(0.25, -0.5, 0.69))
    assert csv_rows(rec, losses=[(0.25, -0.5, 0.69), (1.0, 2.0, 3.0)])[1][9:] == ["1.000000", "2.000000", "3.000000"]
    assert len(CSV_HEADER) == 12
    assert rows[0][:9] == [1, "2.0000", "0.5000", "2.0000", 3, "0.5000", "0.5000", "0.4000", "0.2000"]
    assert rows[1][:9] == [2, "3.0000", "1.0000", "0.0000", 0, "0.0000", "0.0000", "0.0000", "0.0000"]
    assert rows[1][9:] == ["0.250000", "-0.500000", "0.690000"]


def test_rollout_step_argument_checks_without_gpu():
    """uavhip_rollout_step rejects a bad env descriptor, a policy of another architecture and env
    dims beyond the one-env-per-wave layout (N, M <= 64) before any HIP call."""
    import ctypes
    from uavhip import _lib
    d = _lib.EnvDesc()
    d.E, d.N, d.M, d.Kn, d.Ki, d.scene_buffers = 4, 100, 4, 1, 1, 1
    pol = _lib.PolicyDesc()
    args = (None, None, 0, 1, ctypes.c_uint64(0), ctypes.c_uint64(0), None, None, None, None, 1, None, None, None,
            None, None)
    assert _lib.LIB.uavhip_rollout_step(pol, d, *args) == -1
    assert b"bad env dims" in _lib.LIB.uavhip_last_error()
    d.N = 8
    for name in ("uav_pos", "uav_vel", "uav_load", "uav_cost", "tgt_pos", "tgt_vel", "tgt_value", "tgt_id", "nfz_pos",
                 "icp_pos", "icp_vel", "p_dmg", "p_pen", "istate", "nh_final", "nh_pure", "t_cost", "n_lock",
                 "assigned", "dstate", "window"):
        setattr(d, name, 16)  # non-NULL placeholders: validation never dereferences them
    assert _lib.LIB.uavhip_rollout_step(pol, d, *args) == -1
    assert b"uavhip_rollout_step" in _lib.LIB.uavhip_last_error()  # NULL weights / states


def test_range_table_scales():
    """The range table (include/uavhip.h uavhip_policy_range_table, policy_layout.hpp; the packed
    buffer carries its maxima, the kernels derive the rest bitwise the same way): the max |param| of
    every tensor, the layer-0 constants, and for every static
    split-product operand a pair (2^-s, 2^s) -- (1, 1) for the reference's initial weights (results
    bitwise those without scaling), and a power of two putting the operand's bound in [2^14, 2^15)
    when the weights drive it out of [2^-4, 2^15). Each bound holds: the LayerNorm and FFN-hidden
    activations of a torch forward on random windows stay below the bound the table was made from."""
    import numpy as np
    from uavhip.policy import RANGE_FLOATS, TransformerActorCritic, range_table
    torch.manual_seed(4)
    net = TransformerActorCritic()
    sd = list(net.state_dict().values())
    t = range_table(sd).numpy()
    assert t.shape == (RANGE_FLOATS,)
    np.testing.assert_array_equal(t[:50], np.array([float(p.abs().max()) for p in sd], np.float32))
    ops = t[64:84].reshape(10, 2)
    np.testing.assert_array_equal(ops, np.ones((10, 2), np.float32))  # realistic weights: unscaled
    # the critic's layer-0 FFN1 x 1e5: its hidden bound ~1e7 -> s = 9..10; LN1 x 1e-6 -> s < 0; the
    # last LayerNorms (the heads' inputs, static operands 8 / 9 of the weight-gradient GEMM) x 1e5
    c0 = net.critic_net.transformer.layers[0]
    a0 = net.actor_net.transformer.layers[0]
    c1 = net.critic_net.transformer.layers[1]
    with torch.no_grad():
        c0.linear1.weight.mul_(1e5)
        c0.norm1.weight.mul_(1e-6)
        c0.norm1.bias.mul_(1e-6)
        a0.norm2.weight.mul_(1e5)
        c1.norm2.weight.mul_(1e5)
    sd = list(net.state_dict().values())
    t = range_table(sd).numpy()
    ln1 = 11.5 * float(c0.norm1.weight.abs().max()) + float(c0.norm1.bias.abs().max())
    hid = 128 * float(c0.linear1.weight.abs().max()) * ln1 + float(c0.linear1.bias.abs().max())
    ln2a = 11.5 * float(a0.norm2.weight.abs().max()) + float(a0.norm2.bias.abs().max())
    ln2c = 11.5 * float(c1.norm2.weight.abs().max()) + float(c1.norm2.bias.abs().max())
    assert not 2 ** -4 <= ln1 < 2 ** 15  # LN1's output is driven out of the unscaled band
    assert not ln2a < 2 ** 15 and not ln2c < 2 ** 15
    for op, bound in ((2, ln1), (3, hid), (8, ln2a), (9, ln2c)):  # policy_layout.hpp range_op
        sc, inv = t[64 + 2 * op], t[65 + 2 * op]
        assert sc * inv == 1.0 and np.log2(inv) == round(np.log2(inv))
        if 2 ** -4 <= bound < 2 ** 15:
            assert sc == 1.0, (op, bound, sc)
        else:
            assert 2 ** 14 <= bound * sc < 2 ** 15, (op, bound, sc)
    # the bounds are bounds: a forward on random windows never exceeds them
    acts = {}
    c0.norm1.register_forward_hook(lambda m, i, o: acts.__setitem__("ln1", float(o.abs().max())))
    c0.linear1.register_forward_hook(lambda m, i, o: acts.__setitem__("hid", float(o.relu().abs().max())))
    with torch.no_grad():
        net.evaluate(torch.randn(64, 5, 14) * 3, torch.zeros(64, dtype=torch.long))
    assert acts["ln1"] <= ln1 and acts["hid"] <= hid, (acts, ln1, hid)


def test_range_exp_saturates_for_overflowing_bounds():
    """a bound that overflows fp32 (inf, or >= 2^115 -- the bounds are products of
    maxima) takes the largest exponent a finite fp32 operand needs, s = 113 (2^128 x 2^-113 = 2^15),
    instead of turning the scaling off; a NaN maximum leaves s = 0 (non-finite stays non-finite)."""
    import math
    import numpy as np
    from uavhip.policy import TransformerActorCritic, range_table
    net = TransformerActorCritic()
    c0 = net.critic_net.transformer.layers[0]
    with torch.no_grad():
        c0.norm1.weight.fill_(2.0 ** 120 / 11.5)  # LN1's bound ~2^120 (finite, >= 2^115)
        c0.linear1.weight.fill_(2.0 ** 30)       # the FFN hidden bound overflows to inf
    sd = list(net.state_dict().values())
    t = range_table(sd).numpy()
    ln1 = 11.5 * float(c0.norm1.weight.abs().max()) + float(c0.norm1.bias.abs().max())
    assert ln1 >= 2.0 ** 115 and math.isfinite(ln1)
    for op in (2, 3):  # critic layer 0: LN1 output, FFN hidden (policy_layout.hpp range_op)
        sc, inv = float(t[64 + 2 * op]), float(t[65 + 2 * op])
        assert (sc, inv) == (2.0 ** -113, 2.0 ** 113), (op, sc, inv)
    # the unaffected operands keep s = 0
    assert float(t[64 + 2 * 0]) == 1.0 and float(t[64 + 2 * 6]) == 1.0
    # NaN elements do not count in a maximum (the device's fmaxf reductions drop them)
    keys = list(net.state_dict().keys())
    qi = keys.index("critic_net.transformer.layers.1.norm1.weight")
    m = [p.detach().clone() for p in sd]
    m[qi].uniform_(-1, 1)
    m[qi][0] = 3.0
    m[qi][1] = float("nan")
    assert float(range_table(m)[qi]) == 3.0


def test_loader_refuses_a_foreign_library_unless_opted_in(tmp_path):
    """UAVHIP_LIB pointing at a library without the current ABI's entry points fails at
    import (not later, far from the cause); only UAVHIP_ACCEPT_PREV_ABI=1 (the A/B timing scripts)
    relaxes the check, with a warning."""
    import subprocess
    import sys
    lib = os.path.join(ROOT, "oracle", "libuav_oracle.so")  # a shared library with none of the symbols
    if not os.path.exists(lib):
        pytest.skip("oracle library not built")
    pkg = os.path.join(ROOT, "target-allocation-ppo-transformer_amd")
    code = f"import sys; sys.path.insert(0, {pkg!r}); import uavhip._lib"
    env = dict(os.environ, UAVHIP_LIB=lib)
    env.pop("UAVHIP_ACCEPT_PREV_ABI", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "missing entry points" in out.stderr, out.stderr[-400:]
