"""The two builds of tests/device_units/units.hip behind one interface (TEST INFRASTRUCTURE ONLY).

``emu``  libdevice_units_emu.so: the plain C++ twins of the building blocks, on host tensors.
``gpu``  libdevice_units_gfx950.so: the ``__HIP_DEVICE_COMPILE__`` bodies that ship, on cuda tensors (tests marked ``gpu``).  The
         library is the one ``__graft_entry__.build()`` left in the tree; it is rebuilt here only when it is stale and hipcc is
         present, and a test whose library can be neither loaded nor built fails -- it does not skip.

Use as ``@pytest.mark.parametrize("units", BACKENDS, indirect=True)`` after importing ``units`` into the test module.
"""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

from tests.device_units import build as units_build

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]

P, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
SIGNATURES = {                                               # the stream argument comes last everywhere
    "du_fft_plan": [I, I, I, P, P, P, P, P],
    "du_helpers": [I, P, P, I, P],
    "du_wave_f64": [P, P, P, P, I, I, P],
    "du_wave_f32": [P, P, I, I, P],
    "du_wave_u32": [P, P, I, I, P],
    "du_math": [I, P, P, P, L, P],
    "du_phase_term": [P, P, L, D, P],
    "du_buf": [I, P, I, P, P, P, I, P],
}


def cases(argvalues, ids=None):
    """argument sets for ``parametrize("units,<names>", ...)``: every case on the emulator under its own id (the id it had before
    there was a GPU leg) and on the GPU under ``gpu-<id>``"""
    out = []
    for k, a in enumerate(argvalues):
        a = a if isinstance(a, tuple) else (a,)
        name = ids[k] if ids else "-".join(str(x) for x in a)
        out.append(pytest.param("emu", *a, id=name))
    for k, a in enumerate(argvalues):
        a = a if isinstance(a, tuple) else (a,)
        name = ids[k] if ids else "-".join(str(x) for x in a)
        out.append(pytest.param("gpu", *a, id="gpu-" + name, marks=pytest.mark.gpu))
    return out


class Units:
    def __init__(self, name, path, device):
        self.name, self.device = name, device
        self.cdll = ctypes.CDLL(path)
        for fn, args in SIGNATURES.items():
            f = getattr(self.cdll, fn)
            f.restype, f.argtypes = I, args

    def to(self, a):
        """a numpy array as a tensor in the backend's memory"""
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def call(self, fn, *args):
        """tensors go in as raw pointers, the current stream is appended; the entry point must return 0"""
        raw = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
        stream = torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else 0
        rc = getattr(self.cdll, fn)(*raw, stream)
        assert rc == 0, "%s returned %d" % (fn, rc)

    def numpy(self, t):
        return t.cpu().numpy()                               # (a copy off the GPU waits for the stream)


_LOADED = {}


def load(backend):
    if backend in _LOADED:
        return _LOADED[backend]
    if backend == "emu":
        u = Units("emu", units_build.build_emu(), torch.device("cpu"))
    else:
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        if units_build.gpu_stale():
            if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
                pytest.fail("%s is missing or older than its sources and there is no hipcc to build it: run "
                            "__graft_entry__.build() where the tree was built" % units_build.LIB_GPU)
            units_build.build_gpu()
        u = Units("gpu", units_build.LIB_GPU, torch.device("cuda:0"))
    _LOADED[backend] = u
    return u


@pytest.fixture
def units(request):
    return load(request.param)
