"""f64::neg2log_1k on the GPU, bit for bit against the host build of the same header.

Every operation of the function is an fma, an exact integer step or an exact conversion, so the device — the table in
LDS as MathCtx<double>::init<true>() copies it, the inline-assembly fmas, hipcc's own flags — must return the very
bits g++ does; tests/test_neg2log_1k.py holds those to the accuracy bounds.  2^16 arguments: u = 1, u = 2^-53, every
chunk boundary of the 1024-entry table +- 3 ulp, the uniforms next to 1, random uniforms."""
import importlib

import numpy as np
import pytest

import neg2log_1k_harness as h

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def test_device_returns_the_host_bits(tmp_path):
    importlib.import_module("monte-carlo-project-cuda_amd")
    torch.cuda.set_device(0)
    L = h.load_device(h.compile_device(tmp_path))
    u = h.device_inputs()
    n = u.size
    want = h.host_eval(h.compile_host(tmp_path), u, tmp_path)
    d_u = torch.from_numpy(u).cuda()
    d_a = torch.empty(n, dtype=torch.float64, device="cuda")
    assert L.n1k_eval(n, d_u.data_ptr(), d_a.data_ptr()) == 0
    got = d_a.cpu().numpy()
    assert np.all(got > 0)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (bad.size, u[bad[:4]], got[bad[:4]], want[bad[:4]])
    one = u == 1.0
    assert one.sum() == 1 and 0.0 < got[one][0] <= h.BIAS_1K
