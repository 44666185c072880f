"""uavhip -- MI355X-native (gfx950) PPO rollout hot path of the UAV->target allocation reference.

    VecUAVEnv          E envs resident in HBM, stepped by HIP kernels (env.hip)
    TransformerActorCritic  reference-compatible policy; fused forward (policy.hip): fp32-accurate split
                       products on the f16 MFMA, embeddings and heads on the f32 MFMA
    gae                GAE + advantage normalisation on the GPU (gae.hip)
    RolloutEngine      T-step batched rollout (+ RCCL trajectory all-gather)
    PPOAgent           agents/ppo.py API
    AllocationSolver   batched inference: actor-only decode to the episode end, best of K (solve.py)
    TrainingRun        the training loop: rollout + update + diagnostics + evaluation, resumable (fit.py)
    ImitationRun       imitation warm start: teacher-forced episodes of the baseline search (imitate.py)
    load_checkpoint    the reference's torch.save(state_dict) files, older architectures reported

Importing this package loads libuavhip.so and raises if it is missing: there is no CPU fallback.
"""
from ._lib import LIB, UavHipError  # noqa: F401  (loads the HIP library or raises)
from .checkpoint import load_checkpoint, save_checkpoint  # noqa: F401
from .config import Config, cfg  # noqa: F401
from .policy import TransformerActorCritic, pack_weights  # noqa: F401
from .ppo import PPOAgent, gae  # noqa: F401
from .rollout import RolloutEngine, Trajectory  # noqa: F401
from .vec_env import VecUAVEnv  # noqa: F401



def __getattr__(name):
    # solve.py is also a command line (python -m uavhip.solve): imported on first use, so that runpy
    # does not find it in sys.modules already
    if name in ("Allocation", "AllocationSolver", "Constraints"):
        from . import solve
        return getattr(solve, name)
    if name == "TrainingRun":  # fit.py is a command line too (python -m uavhip.fit)
        from . import fit
        return fit.TrainingRun
    if name in ("ImitationRun", "TeacherBatch"):  # and imitate.py (python -m uavhip.imitate)
        from . import imitate
        return getattr(imitate, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["LIB", "UavHipError", "Config", "cfg", "TransformerActorCritic", "pack_weights", "PPOAgent", "gae",
           "RolloutEngine", "Trajectory", "VecUAVEnv", "load_checkpoint", "save_checkpoint", "Allocation",
           "AllocationSolver", "Constraints", "TrainingRun", "ImitationRun", "TeacherBatch"]
