"""patchioner_amd -- MI355X-native implementation of Patch-ioner's captioning hot path.

Public surface mirrors the reference package (``from patchioner import Patchioner``,
R/pyproject.toml:18-25; ``from src.model import Patchioner`` in the eval scripts).
"""
import os as _os

__version__ = "0.1.0"

# Kernel arguments in device memory: a ROCm launch-latency setting that the HIP runtime reads when it initialises (the first HIP call of
# the process), never over the user's own value.  +1.2 % captions/s through the pipeline, nothing on a synchronous forward.  Set HERE --
# not in bench.py alone -- so that API users, the GPU tests and the benchmark run the same configuration (bench.py reports the
# effective value in its line; tests/conftest.py sets it as well, before pytest's collection can touch the GPU).
_os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
# It is PROCESS-WIDE: every HIP user of this process (torch, RCCL) runs with it, and it is read ONCE, when the HIP runtime initialises --
# a process that has made a GPU call before `import patchioner_amd` keeps whatever it started with (the default above then changes
# nothing).  The number of hardware queues is the runtime's own default (4): pipeline.py probes which of its streams really run side by
# side.  INTEGRATION.md, "process-wide settings".


def runtime_already_initialised() -> bool:
    """True when the HIP runtime was up before the defaults above could take effect (best effort: torch's own view of it)."""
    try:
        import sys as _sys
        t = _sys.modules.get("torch")
        return bool(t is not None and t.cuda.is_initialized())
    except Exception:                                   # noqa: BLE001 -- never fail an import over a diagnostic
        return False


_HIP_UP_AT_IMPORT = runtime_already_initialised()


def __getattr__(name):  # lazy: importing the package must not require a GPU or the built library
    if name == "Patchioner":
        from .model import Patchioner
        return Patchioner
    raise AttributeError(name)
