"""The tower optimizer without a GPU: the CPU restatement of its three kernels (tests/tower_optim_ref.py) against torch.optim.AdamW + clip_grad_norm_
in float64 and against torch.amp.GradScaler's scale rule, the two facts that motivate fp32 master weights, and the agreement of the header, the
ctypes table and the Makefile on the new symbols."""
import math
import os
import re

import numpy as np
import pytest
import torch

import tower_optim_ref as ref
import train_bwd_ref
from conftest import REPO, observe

SYMBOLS = ("pclip_tower_grad_sumsq", "pclip_tower_optim_finish", "pclip_tower_adamw")


def test_fma_helper_rounds_once():
    """The restatement's fma against exact rational arithmetic, and on a case where rounding the float64 sum first would round twice."""
    from fractions import Fraction
    gen = torch.Generator().manual_seed(1)
    a, b = torch.randn(2000, generator=gen), torch.randn(2000, generator=gen)
    c = torch.randn(2000, generator=gen) * torch.exp2(torch.randint(-30, 30, (2000,), generator=gen).float())
    for x, y, z, r in zip(a.tolist(), b.tolist(), c.tolist(), ref.fma(a, b, c).tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        lo, hi = np.nextafter(np.float32(r), np.float32(-np.inf)), np.nextafter(np.float32(r), np.float32(np.inf))
        assert abs(Fraction(r) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact)), (x, y, z, r)
    # a b + c = (2^47 - 2^23) + 2^22 - 2^-24: just below the fp32 tie between c (odd) and 2^47 (even); float64 holds the tie itself, so
    # rounding twice gives 2^47
    x, y, z = 2.0 ** 22 * (1 + 2.0 ** -23), 1 - 2.0 ** -23, 2.0 ** 47 - 2.0 ** 23
    assert float(torch.tensor(x, dtype=torch.float64) * y + z) == 2.0 ** 47 - 2.0 ** 23 + 2.0 ** 22
    assert float(ref.fma(torch.tensor(x), torch.tensor(y), torch.tensor(z))) == z


@pytest.mark.parametrize("gmag,lr,clip", ref.MEASURE_CASES)
def test_restatement_against_float64(gmag, lr, clip):
    """Ten restated steps against torch.optim.AdamW + clip_grad_norm_ in float64 on the master weights: the update within C_UPDATE fp32 ulps of
    max(|w|, |update|) (measured, tower_optim_ref.py), every chunk partial within the derived sum-of-squares bound, the norm within half of the
    total's bound plus the roundings of its own fp32 result (sqrt, division and the final cast: 2^-24 covers the one that is not in double)."""
    ratio, norm_rel, part_rel = ref.run_against_float64(gmag, lr, clip)
    print(f"g {gmag:g} lr {lr:g} clip {clip}: update ratio {ratio:.3f} (bound {ref.C_UPDATE}), grad_norm rel {norm_rel:.3e}, partial rel {part_rel:.3e} "
          f"(bound {ref.SUMSQ_REL_BOUND:.3e})")
    observe("tower optimizer restatement: update error / ulp32(max(|w|, |update|))", ratio, ref.C_UPDATE)
    observe("tower optimizer restatement: chunk partial relative error", part_rel, ref.SUMSQ_REL_BOUND)
    assert ratio <= ref.C_UPDATE
    assert part_rel <= ref.SUMSQ_REL_BOUND
    assert norm_rel <= 0.5 * ref.sumsq_bound(1) * (1 + 1e-6) + 2.0 ** -24 + 2.0 ** -52


def test_sumsq_partial_order_and_bound():
    """Ragged sizes and both gradient dtypes: partials within the derived bound of float64; an Inf or NaN makes exactly its own chunk non-finite."""
    gen = torch.Generator().manual_seed(3)
    numels = [1, 7, 8, 9, 4095, 4096, 4097, 2 * 4096 + 3]
    grads = [(torch.randn(n, generator=gen) * 300).half() if i % 2 else torch.randn(n, generator=gen) * 1e-3 for i, n in enumerate(numels)]
    grads[2] = None
    part = ref.chunk_partials(grads, numels)
    assert part.shape == (sum(-(-n // ref.CHUNK) for n in numels),)
    exact = torch.cat([torch.stack([c.double().pow(2).sum() for c in (torch.zeros(n) if g is None else g).split(ref.CHUNK)]) for g, n in zip(grads, numels)])
    rel = ((part.double() - exact).abs() / exact.clamp_min(1e-300)).max()
    assert float(rel) <= ref.SUMSQ_REL_BOUND and float(part[2]) == 0.0
    for bad in (float("inf"), float("nan")):
        g = [None if t is None else t.clone() for t in grads]
        g[-1][-1] = bad
        p2 = ref.chunk_partials(g, numels)
        assert not math.isfinite(float(p2[-1])) and torch.equal(p2[:-1], part[:-1])
        st = ref.finish(p2, ref.new_state(1024.0), 1.0, 0.9, 0.999)
        assert st["found_inf"] == 1 and st["step"] == 0 and st["b1t"] == 1.0 and st["scale"] == 512.0 and st["tracker"] == 0


def test_scale_rule_matches_grad_scaler_exactly():
    """Scale, growth tracker and the count of taken steps against torch.amp.GradScaler over a scripted sequence of clean and overflowed steps."""
    script = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0]
    p = torch.nn.Parameter(torch.zeros(4))
    taken = []
    opt = torch.optim.SGD([p], lr=0.0)
    opt.register_step_post_hook(lambda *_: taken.append(1))
    scaler = torch.amp.GradScaler("cpu", init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    st = ref.new_state(2.0 ** 16)
    part = ref.chunk_partials([torch.ones(4)], [4])
    bad = ref.chunk_partials([torch.tensor([1.0, float("inf"), 1.0, 1.0])], [4])
    for overflow in script:
        scaler.scale(torch.zeros(1))                             # (creates the scaler's scale tensor on first use)
        p.grad = torch.tensor([1.0, float("inf") if overflow else 1.0, 1.0, 1.0])
        scaler.step(opt)
        scaler.update()
        st = ref.finish(bad if overflow else part, st, None, 0.9, 0.999, growth_interval=3)
        assert st["scale"] == float(scaler.get_scale()) and st["tracker"] == int(scaler._growth_tracker) and st["step"] == len(taken), (st, len(taken))
        b1t = 1.0
        for _ in range(st["step"]):
            b1t *= 0.9
        assert st["b1t"] == b1t                                  # one multiplication per taken step, none for a skipped one
    assert st["step"] == script.count(0) and st["scale"] != 2.0 ** 16


def test_fixed_scale_still_skips_an_overflowed_step():
    bad = ref.chunk_partials([torch.tensor([float("nan")])], [1])
    st = ref.finish(bad, ref.new_state(128.0), None, 0.9, 0.999, dynamic=False)
    assert st["found_inf"] == 1 and st["scale"] == 128.0 and st["step"] == 0
    w = torch.ones(1)
    assert ref.update(torch.ones(1), w, w, w, st, 1e-3, 0.0, False)[0] is w


def test_fp16_weight_moves_through_the_master_and_not_without_it():
    """An fp16 weight of 0.25 under a constant gradient at lr = 1e-5: 200 restated steps move it by at least 4 fp16 ulps through the fp32 master; the same
    200 steps of the fp16-state bank optimizer (train_bwd_ref.adamw_step = adamw_f16_kernel) leave it bit-identical."""
    g16 = torch.full((1,), 0.01, dtype=torch.float16)
    master, m, v, st = torch.full((1,), 0.25), torch.zeros(1), torch.zeros(1), ref.new_state(1.0)
    p16, m16, v16 = torch.full((1,), 0.25, dtype=torch.float16), torch.zeros(1, dtype=torch.float16), torch.zeros(1, dtype=torch.float16)
    for step in range(1, 201):
        st = ref.finish(ref.chunk_partials([g16], [1]), st, None, 0.9, 0.999, dynamic=False)
        master, m, v = ref.update(g16, master, m, v, st, 1e-5, 0.01, True)
        train_bwd_ref.adamw_step(p16, g16, m16, v16, 1e-5, step)
    moved = int(torch.tensor(0.25).half().view(torch.int16)) - int(master.half().view(torch.int16))
    print(f"through the master: 0.25 -> {float(master):.8f} = {moved} fp16 ulps; fp16 state: {float(p16)}")
    assert moved >= 4
    assert int(p16.view(torch.int16)) == int(torch.tensor(0.25).half().view(torch.int16))


def test_second_moment_survives_a_small_gradient():
    """g = 1e-4: (1 - b2) g^2 = 1e-11 is zero in fp16 (adamw_f16_kernel's v) and a plain normal number in the fp32 state."""
    g16 = torch.full((1,), 1e-4, dtype=torch.float16)
    st = ref.finish(ref.chunk_partials([g16], [1]), ref.new_state(1.0), None, 0.9, 0.999, dynamic=False)
    _, _, v = ref.update(g16, torch.full((1,), 0.25), torch.zeros(1), torch.zeros(1), st, 1e-5, 0.01, True)
    assert float(v) > 0 and abs(float(v) / (1e-3 * float(g16) ** 2) - 1) < 1e-5
    p16, m16, v16 = torch.full((1,), 0.25, dtype=torch.float16), torch.zeros(1, dtype=torch.float16), torch.zeros(1, dtype=torch.float16)
    train_bwd_ref.adamw_step(p16, g16, m16, v16, 1e-5, 1)
    assert float(v16) == 0.0


def test_header_ctypes_table_and_makefile_agree():
    from proto_clip_amd import _lib
    header = open(os.path.join(REPO, "include", "pclip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    consts = dict(re.findall(r"#define (PCLIP_TOWER_[A-Z0-9_]+) (0x[0-9a-fA-F]+|\d+)", header))
    want = dict(PCLIP_TOWER_CHUNK=_lib.TOWER_CHUNK, PCLIP_TOWER_ROW_BYTES=_lib.TOWER_ROW_BYTES, PCLIP_TOWER_STATE_BYTES=_lib.TOWER_STATE_BYTES,
                PCLIP_TOWER_PARAM_F16=_lib.TOWER_PARAM_F16, PCLIP_TOWER_GRAD_F16=_lib.TOWER_GRAD_F16, PCLIP_TOWER_ALIGNED=_lib.TOWER_ALIGNED,
                PCLIP_TOWER_DECAY=_lib.TOWER_DECAY)
    assert {k: int(v, 0) for k, v in consts.items()} == want and _lib.TOWER_CHUNK == ref.CHUNK
    mk = open(os.path.join(REPO, "proto-clip_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1).split()
    assert "pclip_tower_optim.hip" in srcs
    assert re.search(r"^pclip_tower_optim\.o:.*\n\t.*-ffp-contract=off", mk, flags=re.M)
    from proto_clip_amd import optim
    assert optim.STATE_DTYPE.itemsize == _lib.TOWER_STATE_BYTES and lib.pclip_abi_version() == 1


def test_refusals_need_no_gpu():
    from proto_clip_amd._lib import PclipError
    from proto_clip_amd.optim import TowerAdamW
    with pytest.raises(PclipError, match="not a device tensor"):
        TowerAdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-5)
    with pytest.raises(PclipError, match="max_grad_norm"):
        TowerAdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-5, max_grad_norm=0.0)
