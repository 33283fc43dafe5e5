#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds kernel by kernel: the gate of a refactor that may rename registers but not change what a kernel issues.

    python tools/device_code_diff.py PARENT_DIR NEW_DIR

Each directory holds one `hipcc --cuda-device-only -S` listing per translation unit (NAME.s), built with the flags of proto-clip_amd/csrc/Makefile
(pclip_train, pclip_tower_optim and pclip_preprocess with -ffp-contract=off, as there).  Kernels are matched by name through RENAMES (applied to the mangled
name, length prefix included: no demangler that knows _Float16 ships with every ROCm); the kernel sets must be equal.  Per kernel it prints, and fails on: a change in the count of MFMA, vector-memory, LDS, barrier, transcendental or convert instructions;
any scratch instruction, private segment or VGPR spill (but for a kernel whose every figure equals the parent's: it is the parent's kernel); a change of the LDS size; a change of the waves-per-SIMD step; a total instruction count more than
1 % from the parent's.  Instructions are classified by the prefixes below and nothing else.

A kernel of the new build without a partner of its own name is compared with the parent's kernel that MOVED names for it, in the same listing (several
copies folded into one shared kernel: many old names to one new one, and one old kernel may stand for several instantiations).  Such a pair passes the
same gate but for the total, which is printed and not gated: a shared kernel carries the arguments of all its callers."""
import os
import re
import sys

CLASSES = {"mfma": ("v_mfma",), "vmem": ("global_", "buffer_", "flat_"), "lds": ("ds_",), "barrier": ("s_barrier",),
           "trans": ("v_exp", "v_rcp", "v_rsq", "v_sqrt", "v_log"), "cvt": ("v_cvt",), "scratch": ("scratch_",)}
RENAMES = (("ce_transpose_kernel", "transpose_kernel"), ("logits_norm_rows_kernel", "norm_rows_kernel"), ("ce_norm_rows_kernel", "norm_rows_kernel"))
# short new name -> the short names of the parent's kernels it replaces (csrc/pclip_rows.h: the prompt-row kernels of CoOp, VPT and MaPLe)
MOVED = {"rows_replace_kernel": ("vpt_replace_kernel",),
         # (the grouped slice sums: the kernels' own earlier names too — two stride arguments more are another mangled name — with CoCoOp's first stage and
         # the coupling's dX merge)
         "rows_grad_part_kernel<16>": ("prompt_ctx_grad_part_kernel", "vpt_grad_part_kernel", "rows_grad_part_kernel"),
         "rows_grad_part_kernel<1>": ("prompt_ctx_grad_part_kernel",),
         "rows_grad_sum_kernel": ("prompt_ctx_grad_sum_kernel", "vpt_grad_sum_kernel"),
         # the slice sums with a group flag: the ungrouped instantiations against the kernels' own earlier names, the grouped ones against CoCoOp's first
         # stage and the coupling's dX merge
         "rows_grad_part_kernel<16, false>": ("rows_grad_part_kernel<16>",),
         "rows_grad_part_kernel<1, false>": ("rows_grad_part_kernel<1>",),
         "rows_grad_part_kernel<16, true>": ("cond_grad_part_kernel",),
         "rows_grad_sum_kernel<false>": ("rows_grad_sum_kernel",),
         "rows_grad_sum_kernel<true>": ("couple_dx_sum_kernel",),
         # csrc/pclip_small_linear.h: the coupling function's and the meta-net's layer walks
         "rowdot16_kernel<float, false, true>": ("couple_fwd_kernel",),
         "rowdot16_kernel<half_t, true, false>": ("metanet_l1_kernel",),
         "small_linear_dw_kernel<float>": ("couple_dw_kernel", "metanet_dw_kernel<float>"),
         "small_linear_dw_kernel<half_t>": ("metanet_dw_kernel<half_t>",),
         "small_linear_db_kernel<0>": ("couple_db_kernel", "metanet_db_kernel")}
# the cosine cross-entropy kernels with a group flag (csrc/pclip_cosine_ce.hip, csrc/pclip_panel_walk.h): the ungrouped AND the grouped instantiation against
# the kernel's own earlier name — the grouped one is the same walk behind a base offset
_CE_FORMS = ["ce_fwd_kernel<%s>" % f for f in ("1, 1", "1, 2", "1, 4", "2, 1", "2, 2", "4, 1")]
_CE_FORMS += ["ce_bwd_kernel<%s>" % f for f in ("1, 1, 8", "1, 2, 8", "1, 4, 8", "2, 1, 16", "2, 2, 16", "4, 1, 32")]
_CE_FORMS += ["%s<%d>" % (k, n) for k in ("norm_rows_kernel", "ce_norm_backward_kernel") for n in (1, 2, 4, 8)] + ["transpose_kernel<64>"]
for _f in _CE_FORMS:
    for _flag in ("false", "true"):
        MOVED["%s, %s>" % (_f[:-1], _flag)] = (_f,)
for _f in ("ce_sum_kernel", "ce_sum_chunks_kernel"):
    for _flag in ("false", "true"):
        MOVED["%s<%s>" % (_f, _flag)] = (_f,)
TOTAL_TOL = 0.01


def short(name):
    """kernel<1, 4, 8> from _ZN12_GLOBAL__N_1<len>kernelILi1ELi4ELi8EEEv..., kernel<half_t, true> from ...kernelIDF16_Lb1EEEv...; other names as they are"""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name)
    if not m:
        return name
    base, rest = name[m.end():m.end() + int(m.group(1))], name[m.end() + int(m.group(1)):]
    targs = re.match(r"I((?:f|DF16_|L[a-z]\d+E)+)E", rest)
    if not targs:
        return base
    args = [{"f": "float", "DF16_": "half_t", "Lb0E": "false", "Lb1E": "true"}.get(a, a[2:-1]) for a in re.findall(r"f|DF16_|L[a-z]\d+E", targs.group(1))]
    return "%s<%s>" % (base, ", ".join(args))


def renamed(name):
    for a, b in RENAMES:
        name = re.sub(r"\b%s\b" % a, b, name.replace("%d%s" % (len(a), a), "%d%s" % (len(b), b)))
    return name


def waves_per_simd(regs):                                # 512 registers per lane and SIMD in granules of 8; .vgpr_count is the unified total, AGPRs included
    return min(8, 512 // max(8, (regs + 7) // 8 * 8))


def parse(path):
    """{kernel name: {class: count, "total", "lds_bytes", "private", "spill", "waves"}} of one listing"""
    text = open(path).read()
    meta = {}
    for entry in re.split(r"^  - (?=\.)", text.split("amdhsa.kernels:")[-1], flags=re.M)[1:]:
        kv = dict(re.findall(r"^    (\.\w+):\s+(.+?)\s*$", entry, flags=re.M))     # (the kernel's own keys: its arguments' sit deeper)
        meta[kv[".name"]] = kv
    out = {}
    for name, kv in meta.items():
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, flags=re.M | re.S).group(0)
        ops = [m for m in re.findall(r"^\s+([a-z][a-z0-9_]*)\b", body, flags=re.M)]
        k = {c: sum(op.startswith(p) for op in ops) for c, p in CLASSES.items()}
        k.update(total=len(ops), lds_bytes=int(kv[".group_segment_fixed_size"]), private=int(kv[".private_segment_fixed_size"]),
                 spill=int(kv.get(".vgpr_spill_count", 0)), waves=waves_per_simd(int(kv[".vgpr_count"])))
        out[name] = k
    return out


def compare(parent_dir, new_dir, out=sys.stdout):
    bad = 0
    units = sorted(set(f for d in (parent_dir, new_dir) for f in os.listdir(d) if f.endswith(".s")))
    for unit in units:
        sides = []
        for d in (parent_dir, new_dir):
            p = os.path.join(d, unit)
            sides.append(parse(p) if os.path.exists(p) else {})
        old, new = {renamed(name): k for name, k in sides[0].items()}, sides[1]
        moved = {}                                       # new name -> the parent's name it is compared with
        for name in set(new) - set(old):
            for was in (o for o in set(old) - set(new) if short(o) in MOVED.get(short(name), ())):
                moved[name] = was
        for name in sorted((set(old) | set(new)) - set(moved.values())):
            why = []
            if name not in new or name not in old and name not in moved:
                why.append("only in the %s build" % ("new" if name in new else "parent"))
            else:
                o, n = old[moved.get(name, name)], new[name]
                why += ["%s %d -> %d" % (c, o[c], n[c]) for c in ("mfma", "vmem", "lds", "barrier", "trans", "cvt", "lds_bytes", "waves") if o[c] != n[c]]
                why += ["%s %d" % (c, n[c]) for c in ("scratch", "private", "spill") if n[c] and o != n]
                if name not in moved and abs(n["total"] - o["total"]) > TOTAL_TOL * o["total"]:
                    why.append("total beyond %g %%" % (100 * TOTAL_TOL))
                print("%-22s %-60s total %5d -> %5d (%+.2f %%)  mfma %4d vmem %4d lds %4d bar %2d trans %3d cvt %3d  waves %d  %s" % (
                    unit, short(name) + (" <- " + short(moved[name]) if name in moved else ""), o["total"], n["total"], 100.0 * (n["total"] - o["total"]) / o["total"], n["mfma"], n["vmem"], n["lds"], n["barrier"],
                    n["trans"], n["cvt"], n["waves"], "same" if o == n else "ok" if not why else ""), file=out)
            if why:
                bad += 1
                print("FAIL %s %s: %s" % (unit, short(name), "; ".join(why)), file=out)
    print("%d kernel(s) failed" % bad if bad else "all kernels pass", file=out)
    return bad


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(1 if compare(sys.argv[1], sys.argv[2]) else 0)
