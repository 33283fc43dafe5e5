"""The tolerance of the forward attention (tests/attention_fwd_ref.py) checked without a GPU: a float64 emulation of the kernel's walk with exactly its
documented roundings stays inside it on every input family, and five wrong walks land outside it wherever they differ from the right one."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_fwd_ref as ref                                     # noqa: E402
from conftest import observe                                        # noqa: E402

B, H = 1, 2
LENGTHS = (1, 31, 33, 64, 65, 97, 129, 197, 257, 288, 321, 385)
CASES = [(f, L, c) for f in ref.FAMILIES for L in LENGTHS for c in (False, True) if not c or L <= 288]
_cache = {}


def case(family, L, causal):
    """Inputs, float64 reference and tolerance of a case, computed once."""
    key = (family, L, causal)
    if key not in _cache:
        fn = ref.steep if family == "steep" else ref.FAMILIES[family]
        qkv = fn(B, L, H, seed=1000 + L)
        _cache[key] = (qkv,) + ref.reference(qkv, B, L, H, causal)
    return _cache[key]


def applies(variant, family, L, causal):
    """Where a wrong walk differs from the right one by more than the kernel's own roundings — the only cases left out of the rejection test."""
    if variant in ("stale_sum", "stale_out"):
        # one pair of key tiles (L <= 64) has nothing to rescale; and the maximum has to move after the first pair: the families on which a later pair
        # of key tiles holds scores more than kAttDefer above everything before it
        return L >= 65 and family in ("ramp", "hot25", "hot40", "onehot", "normal")
    if variant == "drop_last_key":
        # `descend` gives its last key the LOWEST score of the row, 12 below the maximum: a weight of e^-12 = 6e-6, under the u11 of the output's own
        # rounding — a kernel that drops it is right to within the bound (L = 1: the only key, its loss leaves 0 / 0)
        if L > 1 and family == "descend":
            return False
        # causal: ONE row per head sees key L - 1, and the fault shows only if that row gives its own key weight — by construction on `ramp` / `creep` (the
        # highest score of the row), `onehot`, `flat` (1 / L) and `hot` (one key in four is of the row's cluster); on N(0, 1.5^2) scores it is a matter of luck
        return not causal or L == 1 or family in ("ramp", "creep", "onehot", "flat", "hot25", "hot40")
    if variant == "mask_off_by_one":
        # L = 1 has no key q + 1; a one-hot row gives key q + 1 no weight, and neither does a `hot` row: token q + 1 belongs to another cluster, whose keys
        # score tens below the row's own
        return causal and family not in ("onehot", "hot25", "hot40") and L >= 2
    raise AssertionError(variant)


@pytest.mark.parametrize("family,L,causal", CASES)
def test_bound_holds_the_documented_roundings(family, L, causal):
    qkv, want, tol = case(family, L, causal)
    stats = {}
    ratio = ref.worst_ratio(ref.emulate(qkv, B, L, H, causal, stats=stats), want, tol)
    print(f"{family} L={L} causal={causal}: emulation at {ratio:.3f} of the bound, {stats}")
    observe(f"attention forward emulation, {family}: |emu - float64| / derived tolerance", ratio, 1.0)
    assert ratio <= 1.0
    assert stats["pmax"] <= 4.0 * (1 + 1e-12)                           # the deferred maximum: probabilities reach 2^kAttDefer, never more


@pytest.mark.parametrize("family,L,causal", CASES)
def test_bound_rejects_wrong_walks(family, L, causal):
    qkv, want, tol = case(family, L, causal)
    stats = {}
    right = ref.emulate(qkv, B, L, H, causal, stats=stats)
    for variant in ("stale_sum", "stale_out", "drop_last_key", "mask_off_by_one"):
        if not applies(variant, family, L, causal):
            continue
        got = ref.emulate(qkv, B, L, H, causal, variant=variant)
        if variant in ("stale_sum", "stale_out") and stats["moves"] == 0:
            # no row of these inputs rescales (at L = 65 the second pair is ONE key, which has to lie kAttDefer above 64 others): the wrong walk IS the right one
            assert torch.equal(got, right), variant
            continue
        rows = slice(L - 1, L) if variant == "drop_last_key" and causal else slice(None)      # causal: the one row that sees key L - 1
        ratio = ref.worst_ratio(got[:, rows], want[:, rows], tol[:, rows])
        print(f"{family} L={L} causal={causal} {variant}: {ratio:.1f} x the bound")
        assert ratio > 1.0, variant


@pytest.mark.parametrize("L,causal", [(L, c) for L in LENGTHS if L >= 129 for c in (False, True) if not c or L <= 288])
def test_bound_rejects_a_maximum_held_from_the_first_pair(L, causal):
    """On `steep` the scores rise by 69 in the log2 domain over the sequence: from L = 129 on, the keys behind the first pair lie more than 16 above it, and
    probabilities taken against the first pair's maximum leave fp16's range.  The right walk stays inside the bound on the same inputs."""
    qkv, want, tol = case("steep", L, causal)
    assert ref.worst_ratio(ref.emulate(qkv, B, L, H, causal), want, tol) <= 1.0
    stats = {}
    ratio = ref.worst_ratio(ref.emulate(qkv, B, L, H, causal, variant="first_tile_only_max", stats=stats), want, tol)
    print(f"steep L={L} causal={causal} first_tile_only_max: {ratio:.1f} x the bound, {stats}")
    assert stats["pmax"] > ref.F16_MAX and ratio > 1.0


def test_every_length_has_a_family_that_rejects():
    """What `applies` leaves out must not hollow the test: every L >= 65 keeps a family on which a stale sum is caught (and below 65 the fault does not
    exist), and every L one on which a dropped last key is."""
    for causal in (False, True):
        for L in LENGTHS:
            if causal and L > 288:
                continue
            assert any(applies("drop_last_key", f, L, causal) for f in ref.FAMILIES), L
            if L >= 65:
                # `onehot` rescales at every such length (row 64's own key, 18 above the rest, sits in the second pair), so the stale walks are caught there
                assert applies("stale_sum", "onehot", L, causal) and applies("stale_out", "onehot", L, causal)
                stats = {}
                ref.emulate(case("onehot", L, causal)[0], B, L, H, causal, stats=stats)
                assert stats["moves"] > 0, L
            if causal and L >= 2:
                assert any(applies("mask_off_by_one", f, L, causal) for f in ref.FAMILIES), L


@pytest.mark.parametrize("L", [129, 197, 385])
def test_families_drive_the_state_machine(L):
    """The inputs do what they are for, in the emulated walk: on `ramp` the rows rescale at every pair of key tiles after the first (nine in ten at least:
    the noise holds a row back here and there; the last pair may be a few keys only and is not counted); on `creep`
    probabilities exceed 1 (a held maximum) and the rows rescale less often than there are pairs, but do rescale; on `flat` and `descend` the first pair's maximum is never left."""
    pairs = (L + 63) // 64
    full = L // 64
    seen = {}
    for family in ("ramp", "creep", "flat", "descend"):
        st = {}
        ref.emulate(case(family, L, False)[0], B, L, H, False, stats=st)
        seen[family] = st
    assert seen["ramp"]["moves"] >= 0.9 * B * H * L * (full - 1)
    assert seen["creep"]["pmax"] > 1.0
    if L >= 197:
        assert 0 < seen["creep"]["moves"] < B * H * L * (pairs - 1)
    assert seen["flat"]["moves"] == 0 and seen["descend"]["moves"] == 0
