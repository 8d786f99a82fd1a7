"""Which build of the pipelined kernel the launcher picks for a run
(hl_encoder.hip pipeline_build_choice, exported as
hl_amd_pipeline_build_choice): a pure host function, no GPU.

Builds, as hl_amd_last_pipeline_build reports them: 0 the one with the
8x8-family helper tasks, 1 the 512-lane one, 2 the 256-lane one
(hl_encoder_t256.hip).  Modes (hl_amd_set_pipeline_build): 0 per run, 1 and 2
forced.
"""
import os
import re

import hartallo_amd
from hl_testlib import ROOT

HEADER = os.path.join(ROOT, "include", "hartallo_amd.h")
LENGTHS = (2, 5, 10, 20, 30, 60, 120, 128, 256, 1024)


def _lib():
    return hartallo_amd.load_library()


def test_lone_picture_keeps_the_helper_build():
    choice = _lib().hl_amd_pipeline_build_choice
    for mode in (0, 1, 2):
        assert choice(mode, 1, 1) == 0
        assert choice(mode, 1, 0) == 1  # helper tasks off: the 512-lane build, never two workgroups per CU


def test_auto_mode_follows_the_threshold():
    lib = _lib()
    choice, t = lib.hl_amd_pipeline_build_choice, lib.hl_amd_pipeline_build_threshold()
    assert t == 0 or t > 1  # 0: the launcher never picks the 256-lane build on its own
    for n in LENGTHS + ((t - 1, t, t + 1) if t else ()):
        if n < 2:  # (a lone picture: above)
            continue
        want = 2 if t and n >= t else 1
        assert choice(0, n, 0) == want, (n, t)


def test_forced_modes_are_honoured():
    choice = _lib().hl_amd_pipeline_build_choice
    for n in LENGTHS:
        assert choice(1, n, 0) == 1
        assert choice(2, n, 0) == 2
        # a run that qualifies for the helper tasks keeps their build: only it has them
        for mode in (0, 1, 2):
            assert choice(mode, n, 1) == 0


def test_invalid_arguments():
    choice = _lib().hl_amd_pipeline_build_choice
    assert choice(-1, 10, 0) == -1
    assert choice(3, 10, 0) == -1
    assert choice(0, 0, 0) == -1


def test_header_and_bindings_declare_the_entries():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib()
    for name, proto in (("hl_amd_set_pipeline_build", r"int32_t\s+hl_amd_set_pipeline_build\s*\(\s*hl_amd_encoder_t\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)"),
                        ("hl_amd_last_pipeline_build", r"int32_t\s+hl_amd_last_pipeline_build\s*\(\s*hl_amd_encoder_t\s*\*\s*\w+\s*\)"),
                        ("hl_amd_pipeline_build_choice", r"int32_t\s+hl_amd_pipeline_build_choice\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)"),
                        ("hl_amd_pipeline_build_threshold", r"int32_t\s+hl_amd_pipeline_build_threshold\s*\(\s*void\s*\)")):
        assert re.search(proto, src), name
        assert name in hartallo_amd.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert hasattr(hartallo_amd.Encoder, "set_pipeline_build") and hasattr(hartallo_amd.Encoder, "last_pipeline_build")
    # a null encoder: an error, not a crash
    assert lib.hl_amd_set_pipeline_build(None, 2) != 0
    assert lib.hl_amd_last_pipeline_build(None) == -1
