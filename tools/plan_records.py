"""Every op of a list of prepared plans as one line of text, for comparing two builds of the library (profiles/op_table_equivalence.md).

Plans are built in the dry runtime (no GPU): tests/plan_audit.py's TEST_PLANS, VARIANT_PLANS and BENCH_PLANS with MLB_F_OPSHAPES, the UNet, ControlNet
and hint plans (mlis_amd_ctx_at 0, 5, 6) of tiny and tinyxl engines with control 1, 2 and 3, and one plan after mlctx_handoffs_off.

  per op:    plan_audit.op_signature, the mlctx_op_info label and flops, mlctx_op_bytes, and every pointer field reduced to what it points into
             (NULL, param:<key>+offset, slab<k>+offset, input:<name>+offset, scratch:<which>+offset, zeroed, arena): addresses differ from run to run,
             what they point into must not
  per plan:  mlctx_handoff_ops, mlctx_ln_fused, mlctx_gn_fused, mlctx_ln_alias_refused, mem_compute, mem_params, mlctx_weight_streaming_info

Run it in the tree of each build and compare the outputs (or their --digest); only the public wrapper is used, so it runs unchanged on earlier commits.
"""
import argparse
import bisect
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pointer_class(plan, p):
    if not p:
        return "NULL"
    for which, (base, n) in sorted(plan.scratch.items()):
        if base <= p < base + n:
            return f"scratch:{which}+{p - base}"
    j = bisect.bisect_right(plan._reg_lo, p)
    for lo, hi, cls, nm in reversed(plan.regions[:j]):
        if lo <= p < hi:
            if cls == "parameter":
                return f"slab{nm[len('weight slab '):]}+{p - lo}" if nm.startswith("weight slab ") else f"param:{nm}+{p - lo}"
            if cls == "input":
                return f"input:{nm}+{p - lo}"
            return "zeroed"
    return "arena"


def snapshot(PA, ctx, name):
    """PA.Plan for its regions and records; the extents are not used here, so the kinds the audit refuses by name (cadd, freeu_*) get none"""
    extents = PA.extents

    def tolerant(op, scratch=None):
        try:
            return extents(op, scratch)
        except PA.Unknown:
            return [], []
    PA.extents = tolerant
    try:
        return PA.Plan(ctx, name)
    finally:
        PA.extents = extents


def plan_lines(PA, L, ctx, name):
    plan = snapshot(PA, ctx, name)
    flops, nbytes = [f for _, f in ctx.op_list()], ctx.op_bytes()
    out = []
    for o in plan.ops:
        ptrs = " ".join(f"{f}={pointer_class(plan, getattr(o.a, f))}" for f, t in o.a._fields_ if t is ctypes.c_void_p)
        out.append(f"{name} op {o.i}: {PA.op_signature(o)!r} label={o.shape_label!r} flops={flops[o.i]!r} bytes={nbytes[o.i]!r} {ptrs}")
    info = ctx.info()
    counts = " ".join(f"{f}={getattr(L, f)(ctx.h)}" for f in ("mlctx_handoff_ops", "mlctx_ln_fused", "mlctx_gn_fused", "mlctx_ln_alias_refused"))
    out.append(f"{name} plan: ops={len(plan.ops)} {counts} mem_compute={info.mem_compute} mem_params={info.mem_params} streaming={ctx.streaming_info()}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the lines to this file")
    ap.add_argument("--digest", action="store_true", help="print only the op count and the SHA-256 of the lines")
    a = ap.parse_args()
    import plan_audit as PA
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import engine as E
    L = E.L()
    for f in ("mlctx_handoff_ops", "mlctx_ln_fused", "mlctx_gn_fused", "mlctx_ln_alias_refused", "mlctx_handoffs_off"):
        getattr(L, f).argtypes = [E.vp]
    L.mlsd_runtime_dry(1)
    lines = []
    for spec in PA.TEST_PLANS + PA.VARIANT_PLANS + PA.BENCH_PLANS:
        b = PA.build(E, spec, PA.MLB_F_OPSHAPES)
        try:
            lines += plan_lines(PA, L, b.ctx, PA.plan_id(spec))
        finally:
            b.close()
    for model in ("tiny", "tinyxl"):
        for control in (1, 2, 3):
            g = E.Generator(model, 128, 128, 1, defer_weights=True, control=bool(control & E.CONTROL_NET), freeu=bool(control & E.CONTROL_FREEU))
            try:
                for i in (0, 5, 6):
                    ctx = g.ctx_at(i)
                    if ctx is not None:
                        lines += plan_lines(PA, L, ctx, f"engine-{model}-control{control}-ctx{i}")
            finally:
                g.destroy()
    spec = PA.BENCH_PLANS[0]
    b = PA.build(E, spec, PA.MLB_F_OPSHAPES)
    try:
        changed = L.mlctx_handoffs_off(b.ctx.h)
        lines.append(f"{PA.plan_id(spec)}-handoffs-off: mlctx_handoffs_off changed {changed} ops")
        lines += plan_lines(PA, L, b.ctx, PA.plan_id(spec) + "-handoffs-off")
    finally:
        b.close()
    L.mlsd_runtime_dry(0)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    n_ops = sum(" op " in l.split(":")[0] for l in lines)
    if a.digest or a.out:
        print(f"{n_ops} ops, {len(lines)} lines, sha256 {hashlib.sha256(text.encode()).hexdigest()}")
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
