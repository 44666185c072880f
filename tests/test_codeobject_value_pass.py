"""CPU build-time guard on the code objects of the deferred-value rollout kernels (rollout_steps.hip):
k_rollout_actor_steps (both env-path instantiations) and k_value_steps within test_codeobject's limits
(spills <= 32 VGPR / 8 SGPR, <= 256 VGPRs, LDS <= 160 KiB), and their MFMA structure pinned for the
reason k_rollout_steps' is: a change of the counts is a structural change of the kernel and comes with
DESIGN.md. k_rollout_actor_steps: the actor's position-4 embedding and head on the f32 MFMA (36), its
one pruned layer as split products (96) -- k_decode_steps' counts. k_value_steps: the critic's
five-position embedding and the head's first layer over the five tiles of a group (180); the ring
GEMM, layer 0, layer 1's K | V and Q GEMMs and the 80-token batched tail as split products (780)."""
import re

import pytest

import test_codeobject as tc

pytestmark = tc.pytestmark

ACTOR_MFMA = (36, 96)
VALUE_MFMA = (180, 780)


def _mfma(asm, name):
    b = tc.body(asm, name)
    return (len(re.findall(r"\bv_mfma_f32_16x16x4_f32\b", b)), len(re.findall(r"\bv_mfma_f32_16x16x32_f16\b", b)))


def test_value_pass_code_objects(tmp_path):
    asm = tc.compile_asm("rollout_steps.hip", tmp_path)
    ks = tc.kernels(asm)
    actor = [k for k in ks if "k_rollout_actor_steps" in k]
    assert len(actor) == 2, actor  # one per env-step path
    for name in actor:
        tc.check_limits(name, ks[name])
        assert _mfma(asm, name) == ACTOR_MFMA, (name, _mfma(asm, name))
    name = next(k for k in ks if "k_value_steps" in k)
    tc.check_limits(name, ks[name])
    assert _mfma(asm, name) == VALUE_MFMA, (name, _mfma(asm, name))
