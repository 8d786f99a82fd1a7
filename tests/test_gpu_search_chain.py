"""The partition search's uniform chain on the GPU (hl_mbcore.h kSearchTab,
search_partition): golden configurations one picture per call and as one
pipelined batch, each with HL_AMD_MEMO unset and 0 (with the memo off every
quad takes the miss path and forms its own addresses from the candidate's
slot).  The configurations: tiny_32x16_qp26 -- every window hits the
[-17, W + 17] clamp; qcif_qp0_me1 -- me_range 1, the window tests disable
diamond points; et_w64_h32_qp36 -- early termination skips partitionings, so
the table is entered at arbitrary j; w480_h272_qp28_me16 -- all
partitionings, 16x16 chains of two rounds.  Streams and every picture's
reconstruction against the reference's goldens.  Tolerance: none."""
import json
import os

import numpy as np
import pytest
import torch

from hartallo_amd import Encoder
from hl_testlib import GOLDEN, GOLDEN_CONFIGS, GOLDEN_ET_CONFIGS, GpuEncoder, first_diff, golden_input, md5

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(GOLDEN, "golden.json")))
NAMES = ["tiny_32x16_qp26", "qcif_qp0_me1", "et_w64_h32_qp36", "w480_h272_qp28_me16"]
CFGS = [next(c for c in GOLDEN_CONFIGS + GOLDEN_ET_CONFIGS if c[0] == n) for n in NAMES]
MEMO = [None, "0"]


@pytest.fixture
def memo_env(monkeypatch):
    """HL_AMD_MEMO as the encoder reads it at creation (HL_AMD_FAM3 at its default)."""
    monkeypatch.delenv("HL_AMD_FAM3", raising=False)

    def set_(v):
        if v is None:
            monkeypatch.delenv("HL_AMD_MEMO", raising=False)
        else:
            monkeypatch.setenv("HL_AMD_MEMO", v)
    return set_


@pytest.mark.parametrize("memo", MEMO, ids=["default", "off"])
@pytest.mark.parametrize("cfg", CFGS, ids=NAMES)
def test_per_call_matches_reference(gpu, memo_env, cfg, memo):
    name, w, h, n, qp, mer, db, gop, seed = cfg
    memo_env(memo)
    clip = golden_input(cfg)
    ref = open(os.path.join(GOLDEN, name + ".264"), "rb").read()
    enc = GpuEncoder(w, h, qp, mer, db, gop, GOLD[name].get("early_term", 0))
    out = b""
    for f in range(n):
        out += enc.encode(clip[f])
        assert md5(np.concatenate(enc.enc.recon())) == GOLD[name]["recon_md5"][f], f"{name}: recon of frame {f}"
    enc.enc.close()
    assert out == ref, f"{name}: first differing byte {first_diff(out, ref)}"


@pytest.mark.parametrize("memo", MEMO, ids=["default", "off"])
@pytest.mark.parametrize("cfg", CFGS, ids=NAMES)
def test_batch_matches_reference(gpu, memo_env, cfg, memo):
    name, w, h, n, qp, mer, db, gop, seed = cfg
    memo_env(memo)
    clip = golden_input(cfg)
    ref = open(os.path.join(GOLDEN, name + ".264"), "rb").read()
    dev = torch.from_numpy(np.ascontiguousarray(clip)).cuda()
    torch.cuda.synchronize()
    ny = w * h
    ptrs = [(dev[i].data_ptr(), dev[i].data_ptr() + ny, dev[i].data_ptr() + ny + ny // 4) for i in range(n)]
    enc = Encoder(w, h, qp, mer, db, gop, GOLD[name].get("early_term", 0))
    out = b"".join(r.annexb() for r in enc.encode_batch_device(ptrs))
    st = enc.last_batch_stats()
    recons = [enc.debug_recon(k) for k in range(n)]
    last = np.concatenate(enc.recon())
    enc.close()
    assert out == ref, f"{name}: first differing byte {first_diff(out, ref)}"
    assert st["fallbacks"] == 0 and st["waits_gave_up"] == 0, st
    for k, r in enumerate(recons):
        if r is not None:
            assert md5(r) == GOLD[name]["recon_md5"][k], f"{name}: recon of frame {k}"
    assert md5(last) == GOLD[name]["recon_md5"][n - 1]
