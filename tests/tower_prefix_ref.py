"""References for the backward of the two embedding stages in front of block 0 (csrc/pclip_embed_bwd.hip), on the CPU:

  * float64 restatements of both backward passes (what the GPU tests grade against);
  * an emulation of the kernels' summation ORDER with fp32 accumulators (numpy float32: one rounded addition per `+`, as the kernels add) — the
    chunked, segmented reduction of dE and the ascending sums of dpos — with two deliberately wrong walks;
  * the tolerances, derived from the rounding points the kernel file lists, never from what a kernel returns.

Tolerances.  u = 2^-24 is the unit roundoff of fp32.  A sum of n exact terms through a chain of m rounded additions is off by at most
m u sum|terms| to first order (gamma_m = m u / (1 - m u); m u < 1e-3 here and the counts below overstate m by at least two, which covers the
second-order term).
  dpos[l, d]: one accumulator over the B sequences, B additions (the first one, 0 + x, is exact)             -> B u sum_b |dx[b, l, d]|
  dE[id, d] : n rows of the id, spread over k chunks: at most n additions inside the chunks, k - 1 merges    -> (n + k) u sum |dx[rows of id, d]|
  absent ids: exactly zero (tolerance 0).
Where the result is rounded once to fp16 (a parameter held in fp16): half an fp16 ulp of the value in addition, 2^-11 |exact|, and 2^-25 absolute in
fp16's subnormal range."""
import numpy as np
import torch

U32 = 2.0 ** -24


def synth_prompts(B, vocab, seed, L=77):
    """SOT, a random body, EOT (the highest id), zero padding: the id histogram of tokenized prompts (one dominant padding run, B-long SOT / EOT runs)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(B, L, dtype=torch.long)
    for i in range(B):
        ln = int(torch.randint(3, min(23, L - 1), (1,), generator=g))
        t[i, 0] = vocab - 2
        t[i, 1:ln] = torch.randint(1, vocab - 2, (ln - 1,), generator=g)
        t[i, ln] = vocab - 1
    return t


def synth_dx(rows, W, seed):
    """fp16 gradient rows spread over three decades, as a gradient stream is."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.logspace(-3, 0, max(rows, 2))[torch.randperm(max(rows, 2), generator=g)][:rows, None]
    return (torch.randn(rows, W, generator=g) * scale).half()


# ---- float64 restatements -----------------------------------------------------------------------------------------------------------------------------

def text_embed_backward64(dx, tokens, V):
    """(dE [V, W], dpos [L, W]) in float64 from dx [B * L, W] and tokens [B, L]: the backward of E[tokens] + pos."""
    B, L = tokens.shape
    d = dx.double()
    dE = torch.zeros(V, d.shape[1], dtype=torch.float64).index_add_(0, tokens.reshape(-1).clamp(0, V - 1), d)
    return dE, d.reshape(B, L, -1).sum(0)


def vit_embed_backward64(dt, B, L):
    """(dcls [W], dpos [L, W], dpatch [B * (L - 1), W]) in float64 from dt [B * L, W]: the backward of cat(cls, patch) + pos."""
    d = dt.double().reshape(B, L, -1)
    return d[:, 0].sum(0), d.sum(0), d[:, 1:].reshape(B * (L - 1), -1)


# ---- the kernels' summation order, fp32 accumulators --------------------------------------------------------------------------------------------------

def emulate_pos_sum(dx, B, L):
    """dpos as the kernels add it: (..((0 + dx[0, l]) + dx[1, l]) + ..), ascending b, one fp32 accumulator per element."""
    x = dx.float().numpy().reshape(B, L, -1)
    acc = np.zeros(x.shape[1:], np.float32)
    for b in range(B):
        acc = (acc + x[b]).astype(np.float32)
    return torch.from_numpy(acc)


def sorted_ids(tokens, V):
    ids, order = torch.sort(tokens.reshape(-1).clamp(0, V - 1), stable=True)
    return ids.numpy(), order.numpy()


def emulate_text_dE(dx, tokens, V, R, variant=None):
    """dE [V, W] fp32 by the documented walk: the stably sorted rows in chunks of R; inside a chunk a run's rows are added in sorted order into one
    accumulator; a run inside one chunk is written directly; a run across chunk boundaries leaves a partial per chunk (slot 0: the run holding the
    chunk's first position, slot 1: the run holding its last) and the partials are added in ascending chunk order, starting from the first.
    variant "drop_tail": the merge forgets the run's last partial; "double_boundary": it adds the run's second partial twice."""
    x = dx.float().numpy()
    N, W = x.shape
    sid, order = sorted_ids(tokens, V)
    dE = np.zeros((V, W), np.float32)
    nch = (N + R - 1) // R
    part = {}
    for c in range(nch):
        r0, r1 = c * R, min(N, c * R + R)
        from_prev = r0 > 0 and sid[r0 - 1] == sid[r0]
        to_next = r1 < N and sid[r1] == sid[r1 - 1]
        cur, first, acc = sid[r0], True, np.zeros(W, np.float32)
        for r in range(r0, r1):
            if sid[r] != cur:
                if first and from_prev:
                    part[c, 0] = acc
                else:
                    dE[cur] = acc
                cur, first, acc = sid[r], False, np.zeros(W, np.float32)
            acc = (acc + x[order[r]]).astype(np.float32)
        if (first and from_prev) or to_next:
            part[c, 0 if first else 1] = acc
        else:
            dE[cur] = acc
    for c in range(nch - 1):
        r0, r1 = c * R, c * R + R
        tid = sid[r1 - 1]
        if sid[r1] != tid:
            continue
        single = sid[r0] == tid
        if single and r0 > 0 and sid[r0 - 1] == tid:
            continue
        c_end = (int(np.searchsorted(sid, tid, side="right")) - 1) // R
        acc = part[c, 0 if single else 1].copy()
        for k in range(c + 1, c_end + 1):
            if variant == "drop_tail" and k == c_end:
                continue
            acc = (acc + part[k, 0]).astype(np.float32)
            if variant == "double_boundary" and k == c + 1:
                acc = (acc + part[k, 0]).astype(np.float32)
        dE[tid] = acc
    return torch.from_numpy(dE)


# ---- tolerances -----------------------------------------------------------------------------------------------------------------------------------------

def tol_pos_sum(dx, B, L):
    """[L, W]: B u sum_b |dx[b, l, d]|."""
    return B * U32 * dx.double().abs().reshape(B, L, -1).sum(0)


def tol_text_dE(dx, tokens, V, R):
    """[V, W]: (n + k) u sum |rows of the id| with n the id's row count and k the number of chunks its run touches; 0 for an absent id."""
    sid, _ = sorted_ids(tokens, V)
    ids = torch.from_numpy(sid)
    absum = torch.zeros(V, dx.shape[1], dtype=torch.float64).index_add_(0, tokens.reshape(-1).clamp(0, V - 1), dx.double().abs())
    n = torch.bincount(ids, minlength=V).double()
    start = torch.from_numpy(np.searchsorted(sid, np.arange(V), side="left"))
    end = torch.from_numpy(np.searchsorted(sid, np.arange(V), side="right"))
    k = torch.where(n > 0, (end - 1).div(R, rounding_mode="floor") - start.div(R, rounding_mode="floor") + 1, torch.zeros_like(start)).double()
    return (n + k)[:, None] * U32 * absum


def tol_f16(exact):
    """Half an fp16 ulp of the exact value (one rounding to fp16), 2^-25 in the subnormal range."""
    return 2.0 ** -11 * exact.double().abs() + 2.0 ** -25


def worst_ratio(got, want, tol):
    """max |got - want| / tol; where tol is 0 the values must be equal (inf otherwise).  A NaN anywhere is inf."""
    err = (got.double() - want.double()).abs()
    if bool(torch.isnan(err).any()):
        return float("inf")
    zero = tol == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / tol[~zero]).max())


# ---- the kernel-level cases of the text embedding backward (shared by the CPU and the GPU tests) ------------------------------------------------------

def text_case(name, R):
    """(dx [B * L, W] fp16, tokens [B, L] int64, V) of a named case; R = the chunk length the runs are laid against."""
    def case(B, L, V, W, tokens, seed):
        return synth_dx(B * L, W, seed), tokens.reshape(B, L).long(), V
    if name == "prompts":                                   # one padding run across a boundary, B-long SOT / EOT runs, singletons
        return case(3, 77, 512, 64, synth_prompts(3, 512, 11), 1)
    if name == "one_id":                                    # 3080 rows of one id: a single run across every chunk
        return case(40, 77, 8, 128, torch.full((40 * 77,), 5), 2)
    if name == "distinct":                                  # 300 rows, 300 ids, shuffled: every run is one row
        return case(4, 75, 300, 64, torch.randperm(300, generator=torch.Generator().manual_seed(3)), 3)
    if name == "ends_on_boundaries":                        # ids = row // R: every run is exactly one chunk
        return case(3, R, 8, 64, torch.arange(3 * R) // R, 4)
    if name == "straddles_boundaries":                      # ids = (row + R // 2) // R: every boundary is crossed
        return case(3, R, 8, 64, (torch.arange(3 * R) + R // 2) // R, 5)
    if name == "one_row":
        return case(1, 1, 16, 64, torch.tensor([9]), 6)
    if name == "chunk_plus_one":                            # R + 1 rows of one id: the second chunk holds one row
        return case(1, R + 1, 4, 64, torch.full((R + 1,), 2), 7)
    if name.startswith("w"):                                # widths of the released text towers (and a second column group: 640 .. 1024)
        return case(2, 77, 512, int(name[1:]), synth_prompts(2, 512, 12), 8)
    if name == "full_vocab":                                # CLIP's vocabulary: 49 408 rows of dE, all but a handful untouched
        return case(2, 77, 49408, 512, synth_prompts(2, 49408, 13), 9)
    raise KeyError(name)


TEXT_CASES = ["prompts", "one_id", "distinct", "ends_on_boundaries", "straddles_boundaries", "one_row", "chunk_plus_one", "w512", "w640", "w768", "w1024",
              "full_vocab"]
CROSSING_CASES = ["prompts", "one_id", "straddles_boundaries", "chunk_plus_one"]      # those in which some run crosses a chunk boundary
VIT_CASES = [(1, 17, 128), (6, 17, 128), (5, 26, 192), (70, 17, 128), (3, 197, 768), (2, 257, 1024)]
