"""CoCoOp on the GPU (proto_clip_amd.cocoop, autograd.MetaNetFn / CondPromptEmbedFn, csrc/pclip_cocoop.hip): the four kernels bit for bit against the CPU
emulations of their documented orders (tests/cocoop_ref.py) and inside the derived tolerances of float64, the ties to CoOp's kernels, the learner against the
reference's own float64 autograd (fixtures of tests/golden/make_golden_cocoop.py, graded at twice the reference's own fp16-chain distance e_ref per tensor, no
floor), chunk borders, NaN containment, composition with an unfrozen tail, and training."""
import math

import pytest
import torch

import cocoop_ref as ref
import coop_ref
from conftest import golden, observe
from spec import SMALL, TINY, trained_like_

pytestmark = pytest.mark.gpu

NAMES = ("ctx", "w1", "b1", "w2", "b2")
PARAMS = ("ctx", "meta_w1", "meta_b1", "meta_w2", "meta_b2")


def make_model(kw, seed, trained=True):
    from proto_clip_amd.clip.model import build_model, random_state_dict
    sd = random_state_dict(seed=seed, **kw)
    if trained:
        sd = trained_like_(sd, seed)
    sd["logit_scale"] = torch.tensor(ref.LOGIT_SCALE, dtype=torch.float32)
    return build_model(sd).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ---- the conditional assembly and its gradient -------------------------------------------------------------------------------------------------------------------

def _operands(B, N, n_ctx, W, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    emb16 = (torch.randn(vocab, W, generator=g) * 0.02).half()
    pos16 = (torch.randn(77, W, generator=g) * 0.01).half()
    ctx = torch.randn(n_ctx, W, generator=g) * 0.02
    pi = torch.randn(B, W, generator=g) * 0.02
    ctx[0, :4] = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 70000.0, -2.0 ** -26])      # ties to even, overflow, underflow
    pi[0, :4] = torch.tensor([2.0 ** -24, -2.0 ** -12, 1.0, 2.0 ** -26])
    return ctx, pi, coop_ref.prompt_tokens(N, n_ctx, vocab, seed + 1), emb16, pos16


@pytest.mark.parametrize("W", [64, 128])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_assembly_and_gradient_follow_the_documented_order(B, W):
    """N in {1, 16, 17, 33} (the slice borders), n_ctx in {1, 4, 16}, L_out = 77 and a short length; n_ctx = 4 also at L_out = 3, where context rows 2 and 3 have
    no row in the stream.  Assembly: the bits of the restatement, inside the tolerance of its three roundings.  Gradient: the bits of the emulated walk for dctx,
    dpi and dshift, inside the derived tolerance of float64; dx is only read; two calls give the same bits."""
    from proto_clip_amd import ops
    vocab = 60
    for N in (1, 16, 17, 33):
        for n_ctx in (1, 4, 16):
            for L in (77, n_ctx + 7) + ((3,) if n_ctx == 4 else ()):
                case = (N, n_ctx, L)
                ctx, pi, tokens, emb16, pos16 = _operands(B, N, n_ctx, W, vocab, 1000 * B + 10 * N + n_ctx)
                tokens[0, 0], tokens[N - 1, 2 + n_ctx if L > 2 + n_ctx else 0] = -3, vocab + 5      # ids outside the vocabulary clamp to its ends
                args = (ctx.cuda(), pi.cuda(), tokens.cuda(), emb16.cuda(), pos16.cuda(), L)
                x = ops.prompt_embed_cond(*args)
                want = ref.prompt_embed_cond(ctx, pi, tokens, emb16, pos16, L)
                assert x.dtype == torch.float16 and x.shape == (B * N * L, W)
                assert torch.equal(bits(x), bits(want)), case
                if L == 77 and N in (1, 17):
                    x64, tol = ref.prompt_embed_cond64(ctx, pi, tokens, emb16, pos16, L)
                    finite = torch.isfinite(want.double())                       # the 70000 overflows to inf in either statement
                    ratio = ref.worst_ratio(x.cpu().double()[finite], x64[finite], tol[finite])
                    observe("prompt_embed_cond: |x - float64| / (tolerance of one fp32 and two fp16 roundings)", ratio, 1.0)
                    assert ratio <= 1.0, (case, ratio)
                    assert torch.equal(bits(ops.prompt_embed_cond(*args)), bits(x))

                dx = ref.synth_dx(B, N, L, W, 7 * B + N + n_ctx + L)
                dxd = dx.cuda()
                got = ops.prompt_cond_grad(dxd, B, N, L, n_ctx)
                emu = ref.emulate_cond_grad(dx, B, N, L, n_ctx)
                tols, f64 = ref.tol_cond_grad(dx, B, N, L, n_ctx), ref.cond_grad64(dx, B, N, L, n_ctx)
                for name, g, e, w, t in zip(("dctx", "dpi", "dshift"), got, emu, f64, tols):
                    assert g.dtype == torch.float32 and g.shape == e.shape, (name, case)
                    assert torch.equal(bits(g), bits(e)), (name, case, float((g.cpu() - e).abs().max()))
                    ratio = ref.worst_ratio(g.cpu(), w, t)
                    observe(f"prompt_cond_grad {name}: |g - float64| / (derived tolerance)", ratio, 1.0)
                    assert ratio <= 1.0, (name, case, ratio)
                assert torch.equal(bits(dxd), bits(dx))                          # the stream is only read
                again = ops.prompt_cond_grad(dxd, B, N, L, n_ctx)
                assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, got)), case
                if L == 3:
                    assert not bits(got[2][:, 2:]).any() and not bits(got[0][2:]).any()      # exact +0 for the rows that do not exist


def test_ties_to_the_shared_context_kernels():
    """pi = 0: the assembly is ops.prompt_embed of the shared context repeated B times.  B = 1: dshift and dctx are ops.prompt_ctx_grad, and dpi is dshift's
    rows added in ascending order."""
    from proto_clip_amd import ops
    W, vocab = 128, 60
    for B, N, n_ctx, L in ((3, 17, 4, 77), (16, 5, 16, 30), (2, 33, 4, 3)):
        ctx, pi, tokens, emb16, pos16 = _operands(B, N, n_ctx, W, vocab, 31 * B + N)
        dev = [t.cuda() for t in (tokens, emb16, pos16)]
        x = ops.prompt_embed_cond(ctx.cuda(), torch.zeros(B, W, device="cuda"), *dev, L)
        assert torch.equal(bits(x), bits(ops.prompt_embed(ctx.cuda(), *dev, L).repeat(B, 1)))
    for N, n_ctx, L in ((1, 4, 9), (16, 4, 77), (17, 16, 30), (33, 4, 3), (100, 4, 12)):
        dx = ref.synth_dx(1, N, L, W, N + L).cuda()
        dctx, dpi, dshift = ops.prompt_cond_grad(dx, 1, N, L, n_ctx)
        shared = ops.prompt_ctx_grad(dx, N, L, n_ctx)
        assert torch.equal(bits(dshift[0]), bits(shared)) and torch.equal(bits(dctx), bits(shared))
        acc = shared[0].clone()
        for j in range(1, min(n_ctx, L - 1)):
            acc = acc + shared[j]
        assert torch.equal(bits(dpi[0]), bits(acc))


@pytest.mark.parametrize("family", ["decades", "cancel"])
@pytest.mark.parametrize("E,Hd,Wt", [(64, 8, 64), (128, 40, 128)])
def test_the_metanet_ties_to_the_coupling_function(E, Hd, Wt, family):
    """The meta-net's layer 1 and its weight / bias gradients are the coupling function's walks (csrc/pclip_small_linear.h) at depth 1 with the B images as the
    rows, B in {1, 3, 16}: h has the bits of relu(ops.couple(f, W1, b1)); dw2, db2 those of ops.couple_backward(dpi, h) and dw1, db1 those of
    ops.couple_backward(dpre, f), dpre from the emulation.  The coupling's envelope wants its input width a multiple of 64: h goes in with zero columns
    appended up to 64 (a column of dWc depends on that column of X alone; dbc on none)."""
    from proto_clip_amd import ops
    for B in (1, 3, 16):
        f, W1, b1, W2, b2, dpi = ref.synth_metanet(B, E, Hd, Wt, 100 * B + Hd, family)
        fd, W1d, b1d, W2d, b2d, dpid = [t.cuda() for t in (f, W1, b1, W2, b2, dpi)]
        h, _ = ops.metanet(fd, W1d, b1d, W2d, b2d)
        pre = ops.couple(fd.float()[None], W1d[None], b1d[None])[0]
        assert torch.equal(bits(h), bits(torch.where(pre <= 0, torch.zeros_like(pre), pre))), B
        dw1, db1, dw2, db2 = ops.metanet_backward(dpid, fd, h, W1d, W2d)
        Hp = (Hd + 63) // 64 * 64
        hp = torch.zeros(B, Hp, device="cuda")
        hp[:, :Hd] = h
        _, dwc, dbc = ops.couple_backward(dpid[None], hp[None], torch.zeros(1, Wt, Hp, device="cuda"), want_x=False)
        assert torch.equal(bits(dw2), bits(dwc[0, :, :Hd])) and torch.equal(bits(db2), bits(dbc[0])), B
        dpre = torch.from_numpy(ref.emulate_metanet_dpre(dpi, h, W2)).cuda()
        _, dwc, dbc = ops.couple_backward(dpre[None], fd.float()[None], W1d[None], want_x=False)
        assert torch.equal(bits(dw1), bits(dwc[0])) and torch.equal(bits(db1), bits(dbc[0])), B


# ---- the meta-net ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["decades", "cancel"])
@pytest.mark.parametrize("E,Hd,Wt", [(64, 4, 64), (128, 8, 128), (640, 40, 512), (1024, 64, 768)])
def test_metanet_follows_the_documented_order(E, Hd, Wt, family):
    """Forward (h, pi) and the four gradients at B in {1, 3, 16}: the bits of the emulation, inside the derived tolerance of float64, the same bits twice; each
    optional gradient alone and all together; the autograd Function over the two entries honours needs_input_grad."""
    from proto_clip_amd import autograd as pag
    from proto_clip_amd import ops
    for B in (1, 3, 16):
        f, W1, b1, W2, b2, dpi = ref.synth_metanet(B, E, Hd, Wt, 100 * B + Hd, family)
        dev = [t.cuda() for t in (f, W1, b1, W2, b2)]
        h, pi = ops.metanet(*dev)
        eh, epi = ref.emulate_metanet_fwd(f, W1, b1, W2, b2)
        assert h.dtype == pi.dtype == torch.float32 and h.shape == (B, Hd) and pi.shape == (B, Wt)
        assert torch.equal(bits(h), bits(eh)), (B, float((h.cpu() - eh).abs().max()))
        assert torch.equal(bits(pi), bits(epi)), (B, float((pi.cpu() - epi).abs().max()))
        _, h64, pi64 = ref.metanet_fwd64(f, W1, b1, W2, b2)
        for name, got, w, t in zip(("h", "pi"), (h, pi), (h64, pi64), ref.tol_metanet_fwd(f, W1, b1, W2, b2)):
            ratio = ref.worst_ratio(got.cpu(), w, t)
            observe(f"metanet forward {name}: |y - float64| / (derived tolerance)", ratio, 1.0)
            assert ratio <= 1.0, (name, B, ratio)
        again = ops.metanet(*dev)
        assert torch.equal(bits(again[0]), bits(h)) and torch.equal(bits(again[1]), bits(pi))
        dpid = dpi.cuda()
        grads = ops.metanet_backward(dpid, dev[0], h, dev[1], dev[3])
        emu = ref.emulate_metanet_bwd(dpi, f, eh, W2)
        for name, got, e, w, t in zip(("dw1", "db1", "dw2", "db2"), grads, emu, ref.metanet_bwd64(dpi, f, eh, W2), ref.tol_metanet_bwd(dpi, f, eh, W2)):
            assert got.dtype == torch.float32 and got.shape == e.shape
            assert torch.equal(bits(got), bits(e)), (name, B, float((got.cpu() - e).abs().max()))
            ratio = ref.worst_ratio(got.cpu(), w, t)
            observe(f"metanet backward {name}: |g - float64| / (derived tolerance)", ratio, 1.0)
            assert ratio <= 1.0, (name, B, ratio)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(ops.metanet_backward(dpid, dev[0], h, dev[1], dev[3]), grads))
        for only in range(4):                                                    # each gradient alone: None for the others, the same bits
            flags = [i == only for i in range(4)]
            part = ops.metanet_backward(dpid, dev[0], h, dev[1], dev[3], *flags)
            assert all((p is None) != fl for p, fl in zip(part, flags)) and torch.equal(bits(part[only]), bits(grads[only]))
        assert ops.metanet_backward(dpid, dev[0], h, dev[1], dev[3], False, False, False, False) == (None, None, None, None)
        # the autograd Function: W1 frozen, no gradient issued for it; the features never get one
        leaves = [dev[0]] + [t.clone().requires_grad_(i != 0) for i, t in enumerate(dev[1:])]
        out = pag.MetaNetFn.apply(*leaves)
        assert torch.equal(bits(out), bits(pi))
        out.backward(dpid)
        assert leaves[1].grad is None and all(torch.equal(bits(leaves[i + 1].grad), bits(grads[i])) for i in (1, 2, 3))


def test_a_hidden_unit_at_exactly_zero_gets_no_gradient_and_a_nan_stays_in_its_image():
    from proto_clip_amd import ops
    f, W1, b1, W2, b2, dpi = ref.synth_metanet(3, 64, 4, 64, 5)
    W1[1], b1[1] = 0.0, 0.0                                                      # unit 1: pre = +0 for every image
    W1[2], b1[2] = 0.0, -0.0                                                     # unit 2: pre = -0
    dev = [t.cuda() for t in (f, W1, b1, W2, b2)]
    h, pi = ops.metanet(*dev)
    assert not bits(h[:, 1]).any() and not bits(h[:, 2]).any()                    # exact +0
    dw1, db1, dw2, db2 = ops.metanet_backward(dpi.cuda(), dev[0], h, dev[1], dev[3])
    assert not bits(dw1[1]).any() and not bits(dw1[2]).any() and not bits(db1[1:3]).any() and not bits(dw2[:, 1:3]).any()
    assert bool(dw1[0].any()) or bool(dw1[3].any())
    bad = f.clone()
    bad[1, 3] = float("nan")
    hb, pib = ops.metanet(bad.cuda(), *dev[1:])
    eh, epi = ref.emulate_metanet_fwd(bad, W1, b1, W2, b2)
    assert bool(torch.isnan(pib[1]).all()) and torch.equal(torch.isnan(hb).cpu(), torch.isnan(eh))
    assert torch.equal(bits(hb[[0, 2]]), bits(h[[0, 2]])) and torch.equal(bits(pib[[0, 2]]), bits(pi[[0, 2]]))


# ---- the learner against the reference ----------------------------------------------------------------------------------------------------------------------------

def make_learner(model, params, tokens, **kw):
    from proto_clip_amd import cocoop
    learner = cocoop.ConditionalPromptLearner([f"class{i}" for i in range(tokens.shape[0])], model, n_ctx=params[0].shape[0], tokenized_prompts=tokens, **kw)
    with torch.no_grad():
        for name, p in zip(PARAMS, params):
            getattr(learner, name).copy_(p.cuda())
    return learner


def fixture_case(name):
    meta = golden(name)
    kw = ref.towers()[str(meta["tag"])]
    assert float(meta["floor"]) == 0.0
    l_eff = int(meta["l_eff"]) or None
    *params, tokens, feats, labels = ref.fixture_inputs(kw, int(meta["B"]), int(meta["N"]), int(meta["n_ctx"]), int(meta["seed"]), l_eff)
    return meta, make_model(kw, int(meta["sd_seed"])), params, tokens, feats.cuda(), labels.cuda()


def run_case(model, params, tokens, feats, labels, loss_scale, truncate=True):
    from proto_clip_amd import cocoop
    learner = make_learner(model, params, tokens, truncate=truncate)
    head = cocoop.CoCoOp(model, learner)
    loss = head.loss(feats, labels)
    (loss * loss_scale).backward()
    with torch.no_grad():
        text = learner(feats)
    return learner, loss, text


@pytest.mark.parametrize("loss_scale", [1.0, 1024.0])
@pytest.mark.parametrize("name", list(ref.FIXTURES))
def test_learner_against_the_reference(name, loss_scale):
    """The text features [B, N, E]: ||t - t64|| / ||t64|| <= 2 e_ref.  Each of the five gradients: ||g - g_f64|| / ||g_f64|| <= 2 e_ref of that tensor (e_ref: the
    reference's own fp16 chain against its float64 run; no floor), the gradient of the 1024-fold loss divided back.  The fixture's ReLU margin guarantees one
    mask for every chain.  Taped and no_grad features are equal bit for bit.  The truncated case also runs at the full context length: the same bits."""
    meta, model, params, tokens, feats, labels = fixture_case(name)
    assert float(meta["relu_min_pre"]) >= ref.RELU_MARGIN * float(meta["relu_max_diff"])
    learner, loss, text = run_case(model, params, tokens, feats, labels, loss_scale)
    assert all(p.grad is None for p in model.parameters())
    taped = learner(feats)
    assert taped.requires_grad and taped.dtype == torch.float16 and taped.shape == (feats.shape[0], tokens.shape[0], model.text_projection.shape[1])
    assert torch.equal(bits(taped), bits(text)) and not text.requires_grad
    t64 = torch.from_numpy(meta["text_f64"]).double()
    worst = {"text": float((text.double().cpu() - t64).norm() / t64.norm()) / (2 * float(meta["text_e_ref"]))}
    observe("cocoop text features: ||t - t64|| / ||t64|| / (2 e_ref)", worst["text"], 1.0)
    for key, pname in zip(NAMES, PARAMS):
        p = getattr(learner, pname)
        assert p.grad.dtype == torch.float32 and p.grad.shape == p.shape
        g, g64 = p.grad.double().cpu() / loss_scale, torch.from_numpy(meta[f"g_{key}_f64"]).double()
        worst[key] = float((g - g64).norm() / g64.norm()) / (2 * float(meta[f"e_ref_{key}"]))
        observe(f"cocoop {key} gradient x{loss_scale:g}: ||g - g64|| / ||g64|| / (2 e_ref)", worst[key], 1.0)
    print(f"{name} x{loss_scale:g}: CoCoOp.loss {float(loss.detach()):.6f}, f64 {float(meta['loss_f64']):.6f}; ratios "
          + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    if int(meta["l_eff"]):
        assert learner.run_length == int(meta["l_eff"])
        full, _, text_full = run_case(model, params, tokens, feats, labels, loss_scale, truncate=False)
        assert full.run_length == 77 and torch.equal(bits(text_full), bits(text))
        for a, b in zip(full.parameters(), learner.parameters()):
            assert torch.equal(bits(a.grad), bits(b.grad))
    assert max(worst.values()) <= 1.0, worst


# ---- chunk borders, NaN containment, composition --------------------------------------------------------------------------------------------------------------------

def small_case(B=3, N=5, n_ctx=4, seed=3, kw=SMALL):
    model = make_model(kw, 31)
    *params, tokens, feats, labels = ref.fixture_inputs(kw, B, N, n_ctx, seed)
    return model, params, tokens, feats.cuda(), labels.cuda()


def test_bits_do_not_depend_on_the_chunk_borders():
    """text_chunk = N (one image per tower pass) against N + 1 (every border but the first falls inside an image) against everything in one pass; more images
    than PCLIP_COCOOP_MAX_B go through in chunks of 16 and give each image the bits it has alone."""
    from proto_clip_amd import cocoop
    model, params, tokens, feats, labels = small_case(B=4, N=5)
    learner = make_learner(model, params, tokens)
    head = cocoop.CoCoOp(model, learner)
    keep = model.text_chunk
    out = {}
    try:
        for chunk in (5, 6, keep):
            model.text_chunk = chunk
            for p in learner.parameters():
                p.grad = None
            (head.loss(feats, labels) * 1024.0).backward()
            with torch.no_grad():
                out[chunk] = (learner(feats), [p.grad.clone() for p in learner.parameters()])
    finally:
        model.text_chunk = keep
    for chunk in (6, keep):
        assert torch.equal(bits(out[chunk][0]), bits(out[5][0])), chunk
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(out[chunk][1], out[5][1])), chunk
    g = torch.Generator().manual_seed(9)
    many = torch.randn(19, SMALL["embed_dim"], generator=g).half().cuda()
    with torch.no_grad():
        text = learner(many)
        assert text.shape == (19, 5, SMALL["embed_dim"])
        for b in (0, 15, 16, 18):
            assert torch.equal(bits(text[b]), bits(learner(many[b:b + 1])[0])), b
    pred = head.classify(many)
    with torch.no_grad():
        from proto_clip_amd import ops, utils
        dense = torch.stack([utils.clip_logits(ops.l2norm_rows(many[b:b + 1]), ops.l2norm_rows(text[b]), scale=float(head.logit_scale()), layout="nd")[0]
                             for b in range(19)])
    assert pred.dtype == torch.int64 and pred.shape == (19,) and torch.equal(pred, dense.argmax(1))
    top, values, indices = head.classify(many, topk=2)
    assert torch.equal(top, pred) and torch.equal(indices[:, 0].long(), pred) and values.shape == (19, 2)


def test_a_nan_in_one_images_features_stays_in_that_images_rows():
    model, params, tokens, feats, labels = small_case(B=3, N=5)
    learner = make_learner(model, params, tokens)
    with torch.no_grad():
        clean = learner(feats)
        bad = feats.clone()
        bad[1, 7] = float("nan")
        text = learner(bad)
    assert bool(torch.isnan(text[1]).all())
    assert torch.equal(bits(text[0]), bits(clean[0])) and torch.equal(bits(text[2]), bits(clean[2]))


def test_composes_with_an_unfrozen_text_block_and_leaves_the_model_untouched():
    from proto_clip_amd import cocoop
    model, params, tokens, feats, labels = small_case()
    with torch.no_grad():
        before = model.encode_text(tokens.cuda())
    learner = make_learner(model, params, tokens)
    head = cocoop.CoCoOp(model, learner)
    (head.loss(feats, labels) * 1024.0).backward()
    assert all(p.grad is None for p in model.parameters())
    frozen = [p.grad.clone() for p in learner.parameters()]
    assert all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in frozen)
    assert torch.equal(model.encode_text(tokens.cuda()), before) and not any(p.requires_grad for p in model.parameters())
    for p in learner.parameters():
        p.grad = None
    model.unfreeze(text_blocks=1)
    (head.loss(feats, labels) * 1024.0).backward()
    last = len(model.transformer.resblocks) - 1
    want = {n for n, _ in model.named_parameters() if n.startswith((f"transformer.resblocks.{last}.", "ln_final.")) or n == "text_projection"}
    for n, p in model.named_parameters():
        if n in want:
            assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape and bool(p.grad.any()), n
        else:
            assert p.grad is None, n
    for p, f in zip(learner.parameters(), frozen):
        assert torch.equal(bits(p.grad), bits(f))                                # the prompts' gradient does not depend on what else is asked for
    # only the meta-net trains: the context gets no gradient, the others keep their bits
    for p in learner.parameters():
        p.grad = None
    learner.ctx.requires_grad_(False)
    (head.loss(feats, labels) * 1024.0).backward()
    assert learner.ctx.grad is None and all(torch.equal(bits(p.grad), bits(f)) for p, f in list(zip(learner.parameters(), frozen))[1:])


def test_refusals_on_the_device_path():
    from proto_clip_amd import ops
    from proto_clip_amd._lib import PclipError
    model, params, tokens, feats, labels = small_case(kw=TINY)
    learner = make_learner(model, params, tokens)
    with ops.low_latency():
        with pytest.raises(PclipError, match="low_latency"):
            learner(feats)
    assert learner(feats).requires_grad
    model.unfreeze(stem="text", heads=False)
    with pytest.raises(PclipError, match=r"text embeddings have been opted in through unfreeze\(stem=\.\.\.\)"):
        learner(feats)
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    with pytest.raises(PclipError, match=r"w2 \(64, 8\) is not \[64, 4\]|do not chain"):
        ops.metanet(z(2, 64).half(), z(4, 64), z(4), z(64, 8), z(64))
    with pytest.raises(PclipError, match=r"b1 \(8,\) is not \[4\]"):
        ops.metanet(z(2, 64).half(), z(4, 64), z(8), z(64, 4), z(64))
    with pytest.raises(PclipError, match=r"expected a float16 tensor"):
        ops.metanet(z(2, 64), z(4, 64), z(4), z(64, 4), z(64))


# ---- training --------------------------------------------------------------------------------------------------------------------------------------------------------

def separable_split(N, K, Q, E, sigma, seed):
    """Unit prototypes per class and samples prototype + sigma * noise / sqrt(E), normalised: (train features [N K, E] fp16, labels), (test [N Q, E], labels)."""
    g = torch.Generator().manual_seed(seed)
    protos = torch.nn.functional.normalize(torch.randn(N, E, generator=g), dim=1)

    def draw(per_class):
        y = torch.arange(N).repeat_interleave(per_class)
        f = protos[y] + sigma * torch.randn(len(y), E, generator=g) / math.sqrt(E)
        return torch.nn.functional.normalize(f, dim=1).half().cuda(), y.cuda()

    return draw(K), draw(Q)


def test_run_cocoop_raises_the_accuracy_of_a_separable_problem():
    """The trainer end to end with its own learner on a SMALL tower: 4 classes of 4 shots around random unit prototypes (sigma 0.5), 8 test images per class,
    8 epochs in batches of 4.  The random tower's text features start unrelated to the prototypes (an accuracy near chance); the learning rate is 5 because the
    context gradient of this seeded tower is about a hundredth of its context's norm (at upstream's 0.002 nothing moves in 32 steps).  The reference's fp32
    chain on the CPU, stepped by the same rule from the same initialisation, goes from 21.9 % to 78.1 %; here the accuracy must rise."""
    from proto_clip_amd import cocoop
    seed, N, n_ctx = 7, 4, 4
    model = make_model(SMALL, 17)
    tokens = coop_ref.prompt_tokens(N, n_ctx, SMALL["vocab_size"], seed)
    (train_f, train_y), (test_f, test_y) = separable_split(N, 4, 8, SMALL["embed_dim"], 0.5, seed)
    cfg = {"cocoop_epochs": 8, "cocoop_batch": 4, "cocoop_lr": 5.0, "seed": seed}
    head = cocoop.run_cocoop(cfg, train_f, train_y, test_f, test_y, [f"class{i}" for i in range(N)], model, tokenized_prompts=tokens)
    res = head.results
    assert isinstance(head, cocoop.CoCoOp) and head.learner.n_ctx == 4 and head.learner.meta_hidden == SMALL["embed_dim"] // 16 and len(res["epochs"]) == 8
    print("run_cocoop: accuracy %.2f -> %.2f, losses %s" % (res["start_test_acc"], res["test_acc"], " ".join(f"{e['loss']:.3f}" for e in res["epochs"])))
    assert all(math.isfinite(e["loss"]) for e in res["epochs"]) and res["epochs"][-1]["loss"] < res["epochs"][0]["loss"]
    assert res["test_acc"] > res["start_test_acc"], res
    pred = head.classify(test_f)
    assert 100.0 * float((pred == test_y).float().mean()) == pytest.approx(res["test_acc"])
    assert not any(p.requires_grad for p in model.parameters())


def test_five_sgd_steps_of_run_cocoop_lower_the_loss():
    """cocoop_ref.SGD_CASE: TINY, 4 images in one batch, 6 classes, 4 context rows, SGD on the five tensors with momentum 0.9 at learning rate 0.1 under a cosine
    schedule over the five steps, loss scale 1024.  The reference's fp32 chain on the CPU, with the fixtures' hook and the same step rule
    (`make_golden_cocoop.py sgd`), goes 1.780782 1.776271 1.768607 1.762200 1.758096 -> 1.756763: a decrease of 0.024019.  At least half of that is required."""
    from proto_clip_amd import cocoop
    tag, sd_seed, B, N, n_ctx, seed, lr = ref.SGD_CASE
    kw = ref.towers()[tag]
    model = make_model(kw, sd_seed)
    *params, tokens, feats, labels = ref.fixture_inputs(kw, B, N, n_ctx, seed)
    feats, labels = feats.cuda(), labels.cuda()
    cfg = {"cocoop_epochs": 5, "cocoop_batch": B, "cocoop_lr": lr, "cocoop_loss_scale": 1024.0, "seed": seed}
    start = make_learner(model, params, tokens)                                  # the measured case starts from the fixture's parameters
    head = cocoop.run_cocoop(cfg, feats, labels, None, None, start.classnames, model, learner=start)
    losses = head.epoch_losses
    assert head.learner is start and len(losses) == 5 and all(math.isfinite(v) for v in losses)
    with torch.no_grad():
        final = float(head.loss(feats, labels))
    print("run_cocoop loss over five SGD steps:", " ".join(f"{v:.6f}" for v in losses), f"-> {final:.6f}; decrease {losses[0] - final:.6f}"
          f" (reference fp32 chain: {ref.SGD_REFERENCE_DECREASE:.6f})")
    observe("run_cocoop: half the reference's five-step decrease / the decrease here", 0.5 * ref.SGD_REFERENCE_DECREASE / max(losses[0] - final, 1e-9), 1.0)
    assert losses[0] - final >= 0.5 * ref.SGD_REFERENCE_DECREASE, (losses, final)
