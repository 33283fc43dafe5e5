"""Every way of running a transformer tower keeps the bits recorded on the commit before the passes were folded into proto_clip_amd/tower.py
(profiles/tower_pass_refactor.txt, `python tests/tower_pass_cases.py --digests`) and, for MaPLe, on the commit before the prompt-row kernels were folded
into csrc/pclip_rows.h (profiles/prompt_rows_refactor.txt): the features of every case of tests/tower_pass_cases.py at TINY and ODD — frozen,
low-latency, heads only, a taped tail behind a frozen prefix, the whole stack, the stem on the tape, CoOp, VPT, MaPLe — and every gradient their
backward produces.  The kernels are deterministic (test_two_runs_give_the_same_bits), so equal call sequences give equal bits."""
import os

import pytest

import tower_pass_cases
from conftest import REPO

pytestmark = pytest.mark.gpu


def recorded_digests():
    out = {}
    for name in ("tower_pass_refactor.txt", "prompt_rows_refactor.txt"):
        for line in open(os.path.join(REPO, "profiles", name)):
            if line.startswith("digest "):
                _, key, value = line.split()
                assert key not in out, key
                out[key] = value
    return out


def test_every_pass_keeps_the_bits_recorded_on_the_parent():
    want = recorded_digests()
    got = tower_pass_cases.gpu_digests()
    assert sum(k.endswith("/features") for k in want) == len(tower_pass_cases.cases(gpu_only=True)) == 48
    assert sum("/grad." in k for k in want) == len(want) - 48 > 0
    assert set(got) == set(want)
    differing = [k for k in want if got[k] != want[k]]
    assert not differing, differing
