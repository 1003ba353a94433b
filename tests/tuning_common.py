"""Shared by the GPU dispatch suites (tests/test_gpu_dispatch.py, tests/test_gpu_dispatch_ext.py):
the tuning keys are process-global, so a test changes one only inside ``with tuned(...)``,
which puts the default back on exit, also when an assertion fails inside the block."""
from vsiquantization_amd import _hip as H

DEFAULTS = {"NONTEMPORAL": 1, "OBS_KERNEL": 0, "LSQ_GROUPS": 0, "PC_PACKED": 1, "K2O_FORM": 0, "K2O_GROUPS": 0,
            "K2O_BLOCK": 0}


def tuned(**knobs):
    """Context manager: set tuning keys (TUNE_<NAME>=value), restore the defaults after."""
    class _T:
        def __enter__(self):
            for k, v in knobs.items():
                H.set_tuning(getattr(H, "TUNE_" + k), v)

        def __exit__(self, *exc):
            for k in knobs:
                H.set_tuning(getattr(H, "TUNE_" + k), DEFAULTS[k])
    return _T()
