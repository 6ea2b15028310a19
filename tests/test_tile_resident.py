"""The training tile kernel's register budget, its hardware-id stamp and the
residency analysis built on it (tools/tile_resident.py).

CPU: the built product library's metadata -- the four band tile kernel
instances use no scratch and at most 64 VGPRs (8 waves per SIMD is what the
kernel's 16 workgroups per CU rest on); the analysis on a hand-made stamp
array whose figures are worked out in the test.
GPU: the stamped instance writes where each tile ran into stamp slot 7.
"""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import REPO, knobs
from gsvc_amd.knobs import Knob

sys.path.insert(0, os.path.join(REPO, "tools"))


def test_product_tile_instances_fit_their_registers():
    import store_hazard_scan as S
    readelf = os.path.join(S.LLVM, "llvm-readelf")
    lib = os.path.join(REPO, "gsvc_amd", "lib", "libgsvc_amd.so")
    assert os.path.exists(lib) and os.path.exists(readelf)
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in S.code_objects(lib, tmp):
            notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True,
                                   check=True).stdout
            for kern in notes.split("\n  - .agpr_count:")[1:]:  # one metadata entry per kernel
                f = dict(re.findall(r"^    (\.[a-z_]+):\s+(\S+)$", kern, flags=re.M))
                if "train_tile_band_kernel" in f.get(".name", ""):
                    found[f[".name"]] = f
    assert len(found) == 4, sorted(found)
    for name, f in found.items():
        assert int(f[".private_segment_fixed_size"]) == 0 and f[".uses_dynamic_stack"] == "false", (name, f)
        assert int(f[".vgpr_spill_count"]) == 0, (name, f)
        assert int(f[".vgpr_count"]) <= 64, (name, f)
        assert int(f[".group_segment_fixed_size"]) <= 10240, (name, f)  # 16 workgroups in 160 KiB


def test_analysis_of_a_hand_made_launch():
    """Four CUs (XCC 0 / 1 x CU 0 / 1) of two slots each, stamps in 10 ns ticks.
    Per CU: tiles A [0, 10] and B [0, 20] us, then C [10, 30] in A's slot at
    once and D [21, 31] in B's slot after 1 us.  So: peak 2 per CU and 8 in
    all; the kernel ends at 31 us; refill waits 0 and 1 us; each CU stands one
    slot empty over [20, 21] and [30, 31], 2 of its 62 slot-us, fill 60 / 62;
    the chip falls below 95 % of 8 for good at 30 us: drain 1 us."""
    import tile_resident as T
    rows = []
    base = 5_000_000
    for xcc in (0, 1):
        for cu in (0, 1):
            for k, (s, e) in enumerate(((0, 1000), (0, 2000), (1000, 3000), (2100, 3100))):
                # wave slot (bits 3:0), SIMD (5:4), pipe (7:6) and the bits above the SE
                # field differ from tile to tile: none of them is part of the CU
                where = (xcc << 32) | (cu << 8) | ((3 * k + cu) & 15) | ((k & 3) << 4) | (1 << 6) | 0x40250000
                rows.append([base + s, 0, 0, 0, base + e, base + e, 20 + k, where])
    r = T.analyze(np.array(rows, dtype=np.int64), "hand")
    assert r["tiles"] == 16 and r["cus"] == 4
    assert r["peak_resident_per_cu"] == {2: 4} and r["peak_resident_total"] == 8
    assert r["kernel_us"] == 31.0
    assert r["ramp_to_peak_us"] == [0.0] * 5
    assert r["slot_refill_wait_us"][0] == 0.0 and r["slot_refill_wait_us"][-1] == 1.0
    assert r["slot_fill"] == round(60 / 62, 4)
    assert r["drain_us"] == 1.0
    assert r["life_us"][0] == 10.0 and r["life_us"][-1] == 20.0
    assert r["entries"][0] == 20.0 and r["entries"][-1] == 23.0


@pytest.mark.gpu
def test_stamped_instance_writes_where_each_tile_ran(cuda):
    """256x256 / 2000 splats, one gradients-only step with the band kernel's
    stamps: every tile has start < end, an XCC id below 8, and the 256
    workgroups -- dealt round-robin over the XCDs -- land on all 8, on 2 to 32
    CUs of each, with SIMD and wave-slot fields in range."""
    from gsvc_amd.frame import make_frame_model, synthetic_gt
    from gsvc_amd.train import train_step_sum
    H = W = 256
    nt = (H // 16) * (W // 16)
    st = torch.zeros((nt, 8), dtype=torch.int64, device=cuda)
    with knobs((Knob.STAMP, 3)) as lib:
        lib.gsvc_debug_set_ptr(ctypes.c_void_p(st.data_ptr()))
        try:
            m = make_frame_model(H, W, 2000, cuda, seed=3)
            g = torch.empty((2000, 9), device=cuda)
            train_step_sum(m._xyz.data, m._cholesky.data, m._features_dc.data, m.rgb_W.data, False,
                           m.cholesky_bound, m.background, synthetic_gt(H, W, 4, cuda).contiguous(),
                           H, W, "L2", grads_out=g)
            torch.cuda.synchronize()
        finally:
            lib.gsvc_debug_set_ptr(None)
    s = st.cpu().numpy()
    assert (s[:, 0] > 0).all() and (s[:, 0] < s[:, 4]).all()
    xcc = s[:, 7] >> 32
    assert sorted(set(xcc.tolist())) == list(range(8)), sorted(set(xcc.tolist()))
    hw = s[:, 7] & 0xffffffff
    cu = (xcc << 8) | ((hw >> 8) & 0xff)
    # 32 workgroups per XCD over its 32 CUs: the SE / SH / CU field names at most
    # 32 CUs per XCD (a field cut from the wrong bits, with wave or SIMD bits in
    # it, names more) and the dispatcher uses more than one of them
    for x in range(8):
        per = len(set(((hw >> 8) & 0xff)[xcc == x].tolist()))
        assert 2 <= per <= 32, (x, per)
    assert len(set(cu.tolist())) <= 256
    # the two waves of a workgroup sit on a CU's 4 SIMDs x 8 slots: SIMD 0-3, slot 0-7 of wave 0
    assert (((hw >> 4) & 3) <= 3).all() and ((hw & 15) <= 7).all(), sorted(set((hw & 15).tolist()))
