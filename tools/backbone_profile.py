#!/usr/bin/env python
"""Per-launch HIP-event table of a model's forward plan, for any YAML at any N x H x W, and the A/B plans of the bottleneck 1x1 convs:

    python tools/backbone_profile.py --config centernet-lightning_amd/configs/resnet50_simple.yaml --batch 32 --size 512 512 [--reps 5] [--all]

Plans (engine._POINTWISE_AB, a tool hook, not a product option):
    (a) default        the shipped plan: cnl_pointwise_nhwc_f32 where the stop rule keeps a shape, conv3 + downsample as ONE two-source launch
    (p) pointwise_all  every stride-1 bottleneck 1x1 conv on cnl_pointwise_nhwc_f32 (what the stop rule is measured from)
    (b) generic_split  every bottleneck 1x1 conv on the generic direct kernel in its split form (CNL_ALGO_FORCE + 5), conv3 and downsample apart
    (c) generic_auto   the generic kernel under its own rule (fp32 matrix cores below 2^20 outputs per image)
Every launch is timed by itself (an event pair around it, the plan replayed in order, median of --reps replays): bench.conv_kernel_profile only knows
the conv entry points of the ResNet-34 plans.  Weights: tests/bottleneck_ref.synth_state_dict (bn3 gamma ~ U(0.1, 0.3): O(1) activations through
33 blocks).  Prints the 1x1 tables of the four plans, the stop-rule table per shape, the three bars of the issue, and images/s of the default plan."""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "centernet-lightning_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import centernet_lightning_amd as cl  # noqa: E402
from centernet_lightning_amd import engine  # noqa: E402

PLANS = [("a", None), ("p", "pointwise_all"), ("b", "generic_split"), ("c", "generic_auto")]
ONE_BY_ONE = re.compile(r"^layer\d\.\d+\.(conv1|conv3|downsample)")


def build(cfg_path, seed=0):
    import bottleneck_ref
    import ref_cpu
    torch.manual_seed(0)
    model = cl.build_centernet(cfg_path)
    if "backbone.layer1.0.conv3.weight" in model.state_dict():
        sd = bottleneck_ref.synth_state_dict(model.state_dict(), seed=seed)
    else:
        sd = ref_cpu.synth_state_dict(model.state_dict(), seed=seed, calib_shape=(2, 3, 128, 128))
    model.load_state_dict(sd)
    return model.cuda()


def plan_of(model, x, mode):
    engine._POINTWISE_AB = mode
    try:
        model._engine.plans.clear()
        model(x)
        torch.cuda.synchronize()
        return model._engine.plan_for(x)
    finally:
        engine._POINTWISE_AB = None


def per_launch(plan, x, reps):
    """-> [(what, us, kind)] in plan order: each launch between its own event pair, the plan replayed `reps` times, the median per launch."""
    stream = torch.cuda.current_stream()
    import ctypes
    cs = ctypes.c_void_p(stream.cuda_stream)
    times = [[] for _ in plan.launches]
    for _ in range(reps + 1):
        outs = {}
        oh, ow = plan.out_hw
        for name, (p, c) in plan.out_params.items():
            t = torch.empty((plan.N, oh, ow, c), device=plan.device)
            p.y = t.data_ptr()
            outs[name] = t
        if plan.absmax is not None:
            plan.absmax.zero_()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(plan.launches) + 1)]
        ev[0].record(stream)
        for i, L in enumerate(plan.launches):
            rc = plan.launch(L, x, cs)
            assert rc == 0, L.what
            ev[i + 1].record(stream)
        torch.cuda.synchronize()
        if _ > 0:                                              # (the first replay warms up)
            for i in range(len(plan.launches)):
                times[i].append(ev[i].elapsed_time(ev[i + 1]) * 1e3)
    lib = plan.lib
    rows = []
    for L, t in zip(plan.launches, times):
        kind = ("pointwise2" if L.aux is not None else "pointwise") if L.fn is lib.cnl_pointwise_nhwc_f32 else \
               ("direct" if L.fn is lib.cnl_conv2d_nhwc_f32 else ("winograd" if L.fn is lib.cnl_conv3x3_winograd_f32 else "other"))
        if L.fn is lib.cnl_conv2d_nhwc_f32:
            kind += "/split" if lib.cnl_conv2d_kernel(ctypes.byref(L.args)) == 5 else "/f32"
        rows.append((L.what, statistics.median(t), kind, L))
    return rows


def forward_ms(model, x, reps):
    for _ in range(3):
        model(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        model(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet50_simple.yaml"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--all", action="store_true", help="print every launch of the default plan, not only the backbone's 1x1 convs")
    a = ap.parse_args()
    model = build(a.config)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(a.batch, 3, *a.size, generator=g).cuda()
    print(f"# {os.path.basename(a.config)}  N={a.batch}  {a.size[0]}x{a.size[1]}  ({torch.cuda.get_device_name()})")
    tabs = {}
    for tag, mode in PLANS:
        plan = plan_of(model, x, mode)
        rows = per_launch(plan, x, a.reps)
        tabs[tag] = rows
        total = sum(r[1] for r in rows)
        sel = [r for r in rows if ONE_BY_ONE.match(r[0])]
        print(f"\n## plan ({tag}) {mode or 'default'}: {len(rows)} launches, sum {total / 1e3:.3f} ms; backbone 1x1 launches {len(sel)}, sum {sum(r[1] for r in sel) / 1e3:.3f} ms")
        for what, us, kind, L in (rows if (a.all and tag == "a") else sel):
            p = L.args
            shp = f"{p.Cin}{'+' + str(L.aux[3]) if L.aux is not None else ''}->{p.Cout} @{p.H_in}x{p.W_in}" if hasattr(p, "Cin") else ""
            print(f"  {what[:62]:62s} {kind:12s} {shp:24s} {us:9.1f} us")
    S = {t: sum(r[1] for r in tabs[t] if ONE_BY_ONE.match(r[0])) for t in tabs}
    print("\n## sums of the backbone 1x1 launches (us)")
    for t, _ in PLANS:
        print(f"  sum({t}) = {S[t]:.1f}")
    print(f"  bar 1: sum(a) <= 0.85 sum(c):  {S['a']:.1f} vs {0.85 * S['c']:.1f}  ->  ratio sum(a)/sum(c) = {S['a'] / S['c']:.3f}  {'MET' if S['a'] <= 0.85 * S['c'] else 'MISSED'}")
    # bar 2: each two-source launch of (a) against its conv3 + downsample pair in (b)
    bt = {r[0].split(" ")[0]: r[1] for r in tabs["b"]}
    print("## bar 2: two-source launch (a) vs conv3 + downsample (b)")
    ok2 = True
    for what, us, kind, L in tabs["a"]:
        if kind == "pointwise2":
            blk = what.split(".conv3")[0]
            pair = bt.get(blk + ".conv3", 0.0) + bt.get(blk + ".downsample", 0.0)
            ok2 &= us < pair
            print(f"  {blk:12s} two-source {us:8.1f} us   conv3 + downsample {pair:8.1f} us   ({us / pair:.3f})")
    print(f"  bar 2 {'MET' if ok2 else 'MISSED'}")
    # stop rule: every single-source shape on the pointwise kernel (p) against the generic split kernel (b), per launch and per shape
    print("## stop rule: single-source 1x1 shapes, pointwise (p) vs generic split (b)  [Cin, Cout, HxW per image]")
    by_shape = {}
    for what, us, kind, L in tabs["p"]:
        if kind == "pointwise":
            p = L.args
            key = (p.Cin, p.Cout, p.H_in, p.W_in)
            by_shape.setdefault(key, [0.0, 0.0, 0])
            by_shape[key][0] += us
            by_shape[key][1] += bt[what.split(" ")[0]]
            by_shape[key][2] += 1
    for key, (up, ub, n) in sorted(by_shape.items()):
        print(f"  Cin {key[0]:5d} Cout {key[1]:5d} {key[2]:4d}x{key[3]:<4d} x{n:2d}: pointwise {up / n:8.1f} us  generic split {ub / n:8.1f} us  "
              f"-> {'pointwise' if up < ub else 'generic'}")
    # bar 3: no shape kept on the pointwise kernel in (a) is slower than in (b)
    worse = [(what, us, bt[what.split(" ")[0]]) for what, us, kind, L in tabs["a"] if kind == "pointwise" and us > bt[what.split(" ")[0]]]
    print(f"## bar 3: single-source launches of (a) slower than in (b): {len(worse)}")
    for w_, u_, b_ in worse:
        print(f"  {w_[:60]:60s} {u_:8.1f} vs {b_:8.1f} us")
    for tag, mode in (("a", None), ("c", "generic_auto")):
        engine._POINTWISE_AB = mode
        model._engine.plans.clear()
        ms = forward_ms(model, x, 10)
        engine._POINTWISE_AB = None
        print(f"## whole forward, plan ({tag}): {ms:.3f} ms per batch of {a.batch}  ->  {a.batch / ms * 1e3:.1f} images/s")
    model._engine.plans.clear()


if __name__ == "__main__":
    main()
