"""bench.py with option "shadow_resume" taken from the environment, for the A/B of profiles/shadow_resume_ab.txt (bench.py itself has no flag for it):

    FLX_SHADOW_RESUME=0 python scripts/bench_shadow_resume.py --gpus 1 --steps 60 --warmup 24 --shadow-split 8
    FLX_HIP_LIB=<another build of libfluctus_hip.so> python scripts/bench_shadow_resume.py --gpus 1 --steps 60 --warmup 24

The option is set right behind every shadow_split that bench.py sets, so it needs --shadow-split K.  When a context is closed, the number of rays its last
split launch suspended goes to stderr ("suspended N"; "n/a" for a library that does not know the option).  Everything else is bench.py, unchanged."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluctus_amd import device  # noqa: E402

_set_option, _close = device.HipContext.set_option, device.HipContext.close


def set_option(self, name, value):
    _set_option(self, name, value)
    if name == "shadow_split" and "FLX_SHADOW_RESUME" in os.environ:
        _set_option(self, "shadow_resume", int(os.environ["FLX_SHADOW_RESUME"]))


def close(self):
    if getattr(self, "h", None):
        try:
            print("suspended", self.get_option("shadow_split_suspended"), file=sys.stderr, flush=True)
        except Exception:
            print("suspended n/a", file=sys.stderr, flush=True)
    _close(self)


device.HipContext.set_option, device.HipContext.close = set_option, close
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
