"""Helpers of the tests that run a stage-D measure in several library calls (a lowered workspace bound) on either host: a spy on
one entry point of the loaded library, a temporary module attribute, and a child process on the torch-free host."""
import contextlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@contextlib.contextmanager
def replaced(owner, name, value):
    """``owner.name = value`` for the duration of the block."""
    old = getattr(owner, name)
    setattr(owner, name, value)
    try:
        yield
    finally:
        setattr(owner, name, old)


@contextlib.contextmanager
def spied(lib, name, *args):
    """The entry point ``name`` of the loaded library wrapped for the duration of the block: yields the list that gets, per call,
    the arguments at the positions ``args`` (one position: the value, several: a tuple)."""
    real, calls = getattr(lib, name), []

    def spy(*a):
        calls.append(int(a[args[0]]) if len(args) == 1 else tuple(int(a[k]) for k in args))
        return real(*a)

    with replaced(lib, name, spy):
        yield calls


CHILD = r"""
import importlib
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
from spectral_connectivity_amd import options
options.precision = sys.argv[2]
scenario = getattr(importlib.import_module(sys.argv[3]), sys.argv[4])
np.savez(sys.argv[6], **scenario(**np.load(sys.argv[5])))
assert "torch" not in sys.modules, "torch was imported"
print("numpy host OK")
"""


def on_torch_free_host(module, scenario, precision, **arrays):
    """``module.scenario(**arrays)`` (a dict of arrays) in a process of its own on the torch-free host (SC_HIP_HOST=numpy), in
    which torch is never imported; returns the dict."""
    with tempfile.TemporaryDirectory() as tmp:
        inp, out = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")
        np.savez(inp, **arrays)
        run = subprocess.run([sys.executable, "-c", CHILD, ROOT, precision, module, scenario, inp, out], cwd=ROOT,
                             env=dict(os.environ, SC_HIP_HOST="numpy"), capture_output=True, text=True, timeout=600)
        assert run.returncode == 0 and "numpy host OK" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
        with np.load(out) as res:
            return {k: res[k] for k in res.files}
