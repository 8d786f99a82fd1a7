"""The memo of the per-block candidate evaluation (hl_mbcore.h kMemoSlots,
eval_candidates) on the GPU: with HL_AMD_MEMO unset (the built capacity), 0
(off) and 8 (a table that overflows at once), one picture per call and as one
pipelined batch, the golden streams and every picture's reconstruction.  The
waves of a workgroup probe and insert unsynchronised inside a pass; the
emulator cannot see that, these runs do.  Tolerance: none."""
import json
import os

import numpy as np
import pytest
import torch

from hartallo_amd import Encoder
from hl_testlib import GOLDEN, GOLDEN_CONFIGS, GOLDEN_ET_CONFIGS, GpuEncoder, first_diff, golden_input, md5

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(GOLDEN, "golden.json")))
NAMES = ["tiny_32x16_qp26", "et_w64_h32_qp36", "qcif_qp12_me2", "w480_h272_qp28_me16"]
CFGS = [next(c for c in GOLDEN_CONFIGS + GOLDEN_ET_CONFIGS if c[0] == n) for n in NAMES]
MEMO = [None, "0", "8"]


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


@pytest.mark.parametrize("memo", MEMO, ids=["default", "off", "8slots"])
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


@pytest.mark.parametrize("memo", MEMO, ids=["default", "off", "8slots"])
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


def test_refuses_bad_setting(gpu, memo_env):
    from hartallo_amd._lib import HL_AMD_ERROR_INVALID_PARAMETER, HlAmdError

    for v in ("3", "-1", "65536"):
        memo_env(v)
        with pytest.raises(HlAmdError) as e:
            Encoder(32, 16)
        assert e.value.code == HL_AMD_ERROR_INVALID_PARAMETER


@pytest.mark.parametrize("memo", [None, "8"], ids=["default", "8slots"])
def test_lone_pictures_with_partitioning_helpers(gpu, memo_env, memo):
    """One P picture per call at 480x272: the 8x8-family partitioning helpers
    run (HL_AMD_FAM3 default), so the recording instantiation of the search
    takes hits, on its own workgroup image."""
    cfg = next(c for c in GOLDEN_CONFIGS if c[0] == "w480_h272_qp28_me16")
    name, w, h, n, qp, mer, db, gop, seed = cfg
    memo_env(memo)
    clip = golden_input(cfg)
    ref = open(os.path.join(GOLDEN, name + ".264"), "rb").read()
    dev = torch.from_numpy(np.ascontiguousarray(clip)).cuda()
    torch.cuda.synchronize()
    ny = w * h
    enc = Encoder(w, h, qp, mer, db, gop)
    out, f3 = b"", 0
    for i in range(n):
        p = dev[i].data_ptr()
        out += enc.encode_device(p, p + ny, p + ny + ny // 4).annexb()
        assert md5(np.concatenate(enc.recon())) == GOLD[name]["recon_md5"][i], f"{name}: recon of frame {i}"
        hs = enc.last_helper_stats()
        f3 += hs.get("fam3_kept", 0) + hs.get("fam3_rejected", 0)
    enc.close()
    assert out == ref, f"{name}: first differing byte {first_diff(out, ref)}"
    assert f3 > 0, "no partitioning helper ran: the case is vacuous"
