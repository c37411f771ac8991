"""GPU: a non-finite image never changes its batch neighbours' bits (include/centernet_gfx950.h at cnl_conv_params.x_absmax and at the decode).

With finite values a leak between images can hide: a neighbour's pixel read through a halo and multiplied by a zero weight, a maximum folded into the
wrong y_absmax line, a tile that spans images and mixes rows in LDS.  With NaN / Inf in ONE image each of them turns a neighbour's bits into NaN — and every
assertion here is an equality of bits or a range check on integers: no tolerance anywhere.

Part A, every launch of every plan.  A plan at N = 3 is replayed twice on the same input through tests/test_gpu_plan_replay.py's stepper.  The clean replay
keeps, for every launch, each image's slice of every declared output view on the device (the tensors of launch_io's `outs`, the image's y_absmax slot
included; flat views — split-K scratch, fuse_part, the reduce's rows — are cut by rows of N H W): the bits themselves, a stronger record than a digest of
them.  The poisoned replay overwrites, AHEAD OF EVERY LAUNCH, image p's slice of every activation input view of that launch (x, the residual, the second
source, the deformable offsets, the fusion inputs, the partial sums, and the fp32 network input for the stem) with a pattern, writes nowhere else, asserts
that the slice holds the pattern, and after the launch compares the OTHER images' slices with the clean replay's: one boolean per launch comes down.
(Poisoning the network input alone would prove little: ReLU is fmaxf, which swallows NaN, so deep launches would never see the poison.)  A launch kind the
io function does not know raises (launch_io), an input view whose name is not listed below raises here.  The 2-D split Winograd kernels winograd5 / 6, which
these plans hardly reach, have a kernel-level case of their own.

Part B, what runs behind the network, at kernel level: cnl_decode_f32 (every stage-1 form and every top-k key storage), the standalone gathers, pack /
unpack, the flip merge, the un-letterbox and the tile merge, with image / frame 1 of 3 poisoned.

Already pinned elsewhere, not repeated here: cnl_track_streams_f32's status words and that a stream with non-finite costs leaves every other stream
untouched (tests/test_gpu_track_streams.py::test_assignment_kernel_status_words, ::test_non_finite_costs_raise_what_tracker_raises_and_leave_every_stream_untouched);
cnl_lsap_batch_f64's status 1 / 2 for a NaN / an unassignable problem beside healthy ones (tests/test_gpu_detection_io.py::test_lsap_segments_with_sentinel_gaps);
the tracker's cost matrices with NaN scores and zero embeddings (tests/test_gpu_tracker.py); the crop and draw kernels' dead slots for NaN / Inf boxes and NaN
scores (the slot tables of tests/test_gpu_crops.py and tests/test_gpu_overlay.py); the tile merge's own rules for NaN boxes and scores
(tests/test_gpu_tiles.py::test_nan_boxes_nan_scores_and_signed_zero_scores_follow_the_rule — here only that a poisoned frame leaves the other frames alone);
winograd9's side-by-side images at kernel level (tests/test_gpu_conv.py::test_winograd9_images_side_by_side_do_not_see_each_other).  The loss kernels are out
of scope: their values are batch sums."""
import ctypes
from collections import OrderedDict

import pytest
import torch

import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib
from centernet_lightning_amd._lib import ConvParams

import test_gpu_bottleneck as bn
import test_gpu_conv as tc
import test_gpu_plan_replay as rp

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
HUGE = 3e38                                 # finite; a sum of two overflows inside the launch


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


# ============================================================================================================================ part A: the plans
def _variant(base, N, H, W):
    cfg, _, _, _, opts, mutate, u8 = rp.PLANS[base] if base in rp.PLANS else rp.SMALL_PLANS[base]
    return (cfg, N, H, W, opts, mutate, u8)


# name -> the PLANS / SMALL_PLANS entry at N = 3 and the smallest frame that still reaches the entry's kernel forms.  C1 / C2 at 256 x 256: maps 64 .. 8,
# so layer3 and layer4 run packed (two images per block row: images 0 and 1 share one, image 2 sits beside an empty half); the tracking model on uint8
# frames (its stem's input cannot be poisoned, every later launch is); F(4,3) needs maps >= 128 pixels wide; resnet50_fpn at 128 x 128: the layer4
# two-source launch has 16 rows per image in one 128-row M tile; latency_split_small at N = 2: the split-K class and its reduce.
SPECS = OrderedDict([
    ("C1", _variant("C1", 3, 256, 256)),
    ("C2", _variant("C2", 3, 256, 256)),
    ("C4", _variant("C4", 3, 96, 160)),
    ("f43", _variant("f43", 3, 256, 512)),
    ("alternate_forms", _variant("alternate_forms", 3, 256, 256)),
    ("f32", _variant("f32", 3, 256, 256)),
] + [(name, _variant(name, 3, 96, 128)) for name in rp.PLANS if name.startswith("neck_")] + [
    ("resnet50_fpn", ("resnet50_fpn.yaml", 3, 128, 128, {}, None, False)),
    ("latency_split_small", _variant("latency_split_small", 2, 256, 256)),
])
SPECS.move_to_end("C1")                 # (the sensitivity tests' plan: the clean record of the last parametrised cases serves them too)

# pattern -> the image it goes to.  (a) all NaN — in every position of the batch; (b) all +Inf; (c) NaN, +Inf, -Inf and +-3e38 from a seeded generator
# (the finite ones overflow inside the launch); (d) finite data whose first and last row and column — the pixels next to a neighbour in memory — are +Inf;
# (e) as (a), with the image's x_absmax slot NaN / +Inf as well, where the launch reads one
PATTERNS = OrderedDict([("nan_p1", ("nan", 1)), ("inf_p1", ("inf", 1)), ("mix_p1", ("mix", 1)), ("border_p1", ("border", 1)), ("nan_slot_nan_p1", ("nan+slot_nan", 1)),
                        ("nan_slot_inf_p1", ("nan+slot_inf", 1)), ("nan_p0", ("nan", 0)), ("nan_p2", ("nan", 2))])
ACTIVATIONS = ("x", "res", "x2", "om", "in0", "in1", "last", "part")       # the input views that hold activations ...
SLOTS = ("xslot", "x2slot")                                               # ... the per-image maxima a launch reads ...
NOT_WRITTEN = ("xfull",)                                                  # ... and the whole buffer a handed-over maximum was taken over (a superset of x)


def _build(name):
    """-> (plan, x, norm, io) of SPECS[name]; the model stays alive with the plan."""
    spec = SPECS[name]
    if name == "resnet50_fpn":
        model, _ = bn._model(spec[0])
        x = rp.structured_images(spec[1], spec[2], spec[3], 50).cuda()
        model._engine.forward(x, sigmoid=True)
        torch.cuda.synchronize()
        plan, norm = next(iter(model._engine.plans.values())), None
    else:
        model, _, plan, x, norm = rp.build_plan(name, spec)
    assert plan.N == spec[1]
    plan._model = model
    pw = plan.lib.cnl_pointwise_nhwc_f32
    return plan, x, norm, (lambda plan_, L, x_, at: bn._pw_io(plan_, L, x_, at) if L.fn is pw else rp.launch_io(plan_, L, x_, at))


def _image(key, v, N, n, hw):
    """Image n's part of a view a launch declares: the first dimension of an NHWC / [n, pixels, c] view, an element of a slot array, and for the flat views
    the image's rows — [slices][N hw][c] (split-K scratch), [blocks][N hw][4] (fuse_part), [N hw][c] (the reduce's output)."""
    if key in ("xslot", "x2slot", "yslot", "slot"):
        assert v.dim() == 1 and v.shape[0] == N, (key, tuple(v.shape))
        return v[n:n + 1]
    if key == "scratch":
        assert v.dim() == 2 and v.shape[0] % (N * hw) == 0, (key, tuple(v.shape), N, hw)
        return v.unflatten(0, (-1, N, hw))[:, n]
    if key == "part":
        assert v.dim() == 3 and v.shape[1] % N == 0, (key, tuple(v.shape))
        return v.unflatten(1, (N, -1))[:, n]
    if v.dim() == 2:                                        # cnl_fused_out_reduce_f32's y: [N hw][c2]
        assert key == "y" and v.shape[0] % N == 0, (key, tuple(v.shape))
        return v.unflatten(0, (N, -1))[n]
    assert v.dim() in (3, 4) and v.shape[0] == N, (key, tuple(v.shape))
    return v[n]


def _out_hw(res):
    y = res.get("y")
    return y.shape[1] * y.shape[2] if y is not None and y.dim() == 4 else 0


def _forms(plan, L, u8):
    """The coverage forms of a launch, as test_the_replayed_plans_reach_every_kernel_form names them (+ the pointwise kernel's)."""
    if L.fn == "stem":
        return {("stem (uint8)" if u8 else "stem") + (" + fused max-pool" if plan.stem_fused_pool else "")}
    if L.fn is plan.lib.cnl_pointwise_nhwc_f32:
        return {"pointwise two-source" if L.aux is not None else "pointwise"}
    if isinstance(L.args, ConvParams):
        form = rp.conv_class(plan.lib, L)[1]
        return {form, form.split(" + ")[0]}
    if isinstance(L.args, _lib.DeconvParams):
        return {"deconv"}
    lib = plan.lib
    for fn, form in ((lib.cnl_fused_out_reduce_f32, "fused_out reduce"), (lib.cnl_depthwise3x3_nhwc_f32, "depthwise"), (lib.cnl_deform_sample_nhwc_f32, "deform sample"),
                     (lib.cnl_upsample2x_nhwc_f32, "upsample"), (lib.cnl_fuse_sum_nhwc_f32, "fuse_sum"), (lib.cnl_absmax_per_image_f32, "absmax pass")):
        if L.fn is fn:
            return {form}
    return {str(L.fn)}


def _zero_scratch(i, L, ins, res):
    """Both replays, as tests/test_gpu_plan_replay.py's lock-step replay: slices of splitk_scratch that the launcher drops as empty are never written, so the
    scratch — an output the launch owns — starts from zeros and the partial sums are part of the comparison."""
    if "scratch" in res:
        res["scratch"].zero_()


def clean_record(plan, x, norm, io):
    """The clean replay -> per launch, {(view name, image): a device clone of that image's part of the view}."""
    rec, N = [], plan.N

    def keep(i, L, ins, res):
        hw = _out_hw(res)
        rec.append({(k, n): _image(k, v, N, n, hw).clone() for k, v in res.items() for n in range(N)})

    rp.replay(plan, x, norm, before=_zero_scratch, after=keep, io=io)
    assert len(rec) == len(plan.launches)
    return rec


def _pattern(kind, shape, gen, is_map):
    """The pattern of one image's part of an input view, on the device.  is_map: the part is an [H, W, C] map (else rows of pixels)."""
    if kind == "nan":
        return torch.full(shape, NAN, device="cuda")
    if kind == "inf":
        return torch.full(shape, INF, device="cuda")
    if kind == "mix":
        table = torch.tensor([NAN, INF, -INF, HUGE, -HUGE], device="cuda")
        return table[torch.randint(0, 5, shape, device="cuda", generator=gen)]
    assert kind == "border", kind
    t = torch.rand(shape, device="cuda", generator=gen)
    if is_map:
        t[0], t[-1] = INF, INF
        t[:, 0], t[:, -1] = INF, INF
    else:                                                       # rows of pixels without a map around them: the first and the last
        t.view(-1, shape[-1])[0] = INF
        t.view(-1, shape[-1])[-1] = INF
    return t


def poisoned_replay(plan, x, norm, io, clean, kind, p, u8=False, after=None, restore=None):
    """The poisoned replay -> (flagged, stats): flagged = [(launch index, what, view name, image)] for every view of an image other than p whose bits differ
    from the clean replay's (in launch order: the first entry is the first launch that differs), stats = launches checked, launches whose input was
    poisoned, launches that returned image p all finite, the forms reached.  after / restore(i, L, ins, res): the sensitivity tests' hooks — `after` runs
    ahead of the comparison, `restore` behind it."""
    N = plan.N
    kind, _, slot = kind.partition("+slot_")
    gen = torch.Generator(device="cuda").manual_seed(1000 + p)
    flagged, stats = [], {"launches": 0, "poisoned": 0, "finite": 0, "forms": set()}
    xp = x.clone()                                              # the stem's input is poisoned in a copy: the clean record's input stays what it was

    def before(i, L, ins, res):
        _zero_scratch(i, L, ins, res)
        done = {}
        for k, v in ins.items():
            if k in NOT_WRITTEN or k in SLOTS:
                continue
            assert k in ACTIVATIONS, f"launch {i} {L.what}: input view {k!r} is not a known activation input"
            if v.dtype != torch.float32:
                assert L.fn == "stem" and v.dtype == torch.uint8, (L.what, k, v.dtype)
                continue                                            # uint8 frames hold no NaN: this launch's input cannot be poisoned
            part = _image(k, v, N, p, _out_hw(res))
            ident = (part.data_ptr(), tuple(part.shape), tuple(part.stride()))
            if ident not in done:                                   # (one buffer under two names gets one pattern)
                if L.fn == "stem":                                  # the network input is NCHW: the pattern of an [H, W, 3] map, seen channels first
                    done[ident] = _pattern(kind, (part.shape[1], part.shape[2], part.shape[0]), gen, True).permute(2, 0, 1)
                else:
                    done[ident] = _pattern(kind, tuple(part.shape), gen, v.dim() == 4)
                part.copy_(done[ident])
        for k in SLOTS:
            if slot and k in ins:
                ins[k][p] = NAN if slot == "nan" else INF
        ok = [torch.ones((), dtype=torch.bool, device="cuda")]
        for k, v in ins.items():
            if k in ACTIVATIONS and v.dtype == torch.float32:
                part = _image(k, v, N, p, _out_hw(res))
                ok.append((_bits(part) == _bits(done[(part.data_ptr(), tuple(part.shape), tuple(part.stride()))])).all())
            if k in SLOTS and slot:
                ok.append(torch.isnan(ins[k][p]) if slot == "nan" else ins[k][p] == INF)
        assert bool(torch.stack(ok).all()), f"launch {i} {L.what}: image {p}'s input does not hold the pattern ahead of the launch"
        stats["poisoned"] += bool(done)

    def check(i, L, ins, res):
        if after is not None:
            after(i, L, ins, res)
        hw = _out_hw(res)
        same = {(k, n): (_bits(_image(k, v, N, n, hw)) == _bits(clean[i][(k, n)])).all() for k, v in res.items() for n in range(N) if n != p}
        assert same, L.what
        main = "y" if "y" in res else "slot"                        # (cnl_absmax_per_image_f32 writes its slots only)
        all_same, finite = torch.stack([torch.stack(list(same.values())).all(), torch.isfinite(_image(main, res[main], N, p, hw)).all()]).tolist()
        if not all_same:                                            # (one download per launch; the names only when something differs)
            flagged.extend((i, L.what, k, n) for (k, n), s in same.items() if not bool(s))
        stats["launches"] += 1
        stats["finite"] += finite
        stats["forms"] |= _forms(plan, L, u8)
        if restore is not None:
            restore(i, L, ins, res)

    rp.replay(plan, xp, norm, before=before, after=check, io=io)
    assert stats["launches"] == len(plan.launches)
    return flagged, stats


_CACHE = {}                     # the plan of the case that ran last and its clean record: the cases run plan by plan
FORMS_REACHED = {}              # plan name -> the forms its poisoned replays reached


@pytest.fixture(scope="module", autouse=True)
def _release_the_cached_plan():
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _plan_and_clean(name):
    if name not in _CACHE:
        _CACHE.clear()
        torch.cuda.empty_cache()
        plan, x, norm, io = _build(name)
        _CACHE[name] = (plan, x, norm, io, clean_record(plan, x, norm, io))
    return _CACHE[name]


def _report(flagged):
    return "\n".join(f"launch {i} {what}: {view} of image {n} differs from the clean replay" for i, what, view, n in flagged[:12])


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("name", list(SPECS))
def test_a_non_finite_image_changes_no_bit_of_its_neighbours_at_any_launch(name, pattern, capsys):
    kind, p = PATTERNS[pattern]
    plan, x, norm, io, clean = _plan_and_clean(name)
    if p >= plan.N:
        p = plan.N - 1                                          # (the N = 2 plan: its last image)
    flagged, stats = poisoned_replay(plan, x, norm, io, clean, kind, p, u8=SPECS[name][6])
    with capsys.disabled():
        print(f"\n[non-finite {name} / {pattern}] image {p} of {plan.N}: {stats['launches']} launches checked, {stats['poisoned']} with a poisoned input, "
              f"{stats['finite']} returned image {p} all finite; flagged {len(flagged)}")
    FORMS_REACHED.setdefault(name, set()).update(stats["forms"])
    assert stats["poisoned"] >= stats["launches"] - (1 if SPECS[name][6] else 0)           # every launch but a uint8 stem
    assert not flagged, f"first launch that differs: launch {flagged[0][0]} {flagged[0][1]}, view {flagged[0][2]}\n" + _report(flagged)


def test_the_poisoned_replays_reach_every_required_kernel_form(capsys):
    """The union of kernel forms over the poisoned replays covers REQUIRED_FORMS of test_the_replayed_plans_reach_every_kernel_form (which exempts nothing of
    that set), the fp32 sub-pixel phases it asks for besides, and the kinds of launch that are no conv.  Plans whose replays did not run in this process
    are built here and their launches counted as they stand."""
    reached = {k: set(v) for k, v in FORMS_REACHED.items()}
    for name in SPECS:
        if name not in reached:
            plan, _, _, _ = _build(name)
            reached[name] = set().union(*(_forms(plan, L, SPECS[name][6]) for L in plan.launches))
            del plan
            torch.cuda.empty_cache()
    forms = set().union(*reached.values())
    with capsys.disabled():
        print("\n[non-finite] forms reached:", sorted(forms))
    want = rp.REQUIRED_FORMS | {"sub-pixel phases fp32", "pointwise two-source", "fused_out reduce", "depthwise", "deform sample", "upsample", "fuse_sum", "deconv",
                                "absmax pass"}
    assert not want - forms, (sorted(want - forms), sorted(forms))
    assert "split-K" in reached["latency_split_small"]           # (at N = 2 the options still take the split-K class: no kernel-level case is needed for it)


# ---------------------------------------------------------------------------------------------------------------------------- sensitivity
SENS = "C1"


def _targets(plan):
    """(a row-Winograd launch that fills a y_absmax slot, its index) — the first of the plan."""
    for i, L in enumerate(plan.launches):
        if isinstance(L.args, ConvParams) and L.args.y_absmax and L.fn is plan.lib.cnl_conv3x3_winograd_f32:
            return i
    raise AssertionError("no Winograd launch that fills a slot")


def test_one_poisoned_element_in_a_neighbour_flags_that_launch_only():
    """After one launch an `after` hook copies ONE element of the poisoned image's output into image 0's: that launch is flagged, for y of image 0, and (the
    element put back behind the comparison) no other."""
    plan, x, norm, io, clean = _plan_and_clean(SENS)
    target = _targets(plan)
    saved = {}

    def after(i, L, ins, res):
        if i == target:
            saved["v"] = res["y"][0, 3, 5, 7].clone()
            res["y"][0, 3, 5, 7] = ins["x"][1, 0, 0, 0]             # (a NaN: what the poisoned image's input holds)

    def restore(i, L, ins, res):
        if i == target:
            res["y"][0, 3, 5, 7] = saved["v"]

    flagged, _ = poisoned_replay(plan, x, norm, io, clean, "nan", 1, after=after, restore=restore)
    assert flagged == [(target, plan.launches[target].what, "y", 0)], flagged


def test_one_ulp_in_a_neighbours_absmax_slot_flags_that_launch_only():
    """... and one ulp added to image 2's y_absmax slot behind a launch: that launch, for the slot of image 2, and no other."""
    plan, x, norm, io, clean = _plan_and_clean(SENS)
    target = _targets(plan)

    def after(i, L, ins, res):
        if i == target:
            res["yslot"].view(torch.int32)[2] += 1

    def restore(i, L, ins, res):
        if i == target:
            res["yslot"].view(torch.int32)[2] -= 1

    flagged, _ = poisoned_replay(plan, x, norm, io, clean, "nan", 1, after=after, restore=restore)
    assert flagged == [(target, plan.launches[target].what, "yslot", 2)], flagged


def test_without_the_hooks_nothing_is_flagged():
    plan, x, norm, io, clean = _plan_and_clean(SENS)
    flagged, stats = poisoned_replay(plan, x, norm, io, clean, "nan", 1)
    assert not flagged and stats["launches"] == len(plan.launches), _report(flagged)


# ---------------------------------------------------------------------------------------------------------------------------- kernel level: winograd5 / 6
@pytest.mark.parametrize("variant,shape", [(5, (3, 32, 32)), (5, (3, 19, 33)), (6, (3, 19, 34)), (6, (3, 9, 20))], ids=lambda t: str(t))
def test_the_2d_split_winograd_kernels_beside_a_non_finite_image(variant, shape):
    """winograd5 serves no launch of the plans above and winograd6 only their packed layer4 maps: at kernel level (tests/test_gpu_conv.py's run_winograd, the
    shapes of its batch-invariance tests — winograd6 lays the images of these maps side by side, so work items span two images), image 1 of 3 non-finite in x
    and in the residual, with the maxima handed over: images 0 and 2 keep the bits of y and of their max |y|."""
    N, H, W = shape
    g = torch.Generator().manual_seed(variant * 100 + W)
    x = torch.randn(N, 128, H, W, generator=g).clamp_min(0) * torch.tensor([1.0, 1e-3, 300.0]).view(N, 1, 1, 1)
    w = torch.randn(256, 128, 3, 3, generator=g) * (2.0 / (128 * 9)) ** 0.5
    b = torch.randn(256, generator=g)
    res = torch.randn(N, 256, H, W, generator=g)
    q = ConvParams()
    q.N, q.H_in, q.W_in, q.Cin, q.Cout, q.KH, q.KW, q.stride, q.pad, q.ldx, q.ldy, q.ldr = N, H, W, 128, 256, 3, 3, 1, 1, 128, 256, 256
    q.flags, q.y, q.x_absmax, q.residual, q.algo = tc.CNL_RELU, 1 << 20, 1 << 20, 1 << 20, tc.CNL_ALGO_FORCE + variant
    assert _lib.load().cnl_conv3x3_winograd_variant(ctypes.byref(q)) == variant
    want, wm = tc.run_winograd(x, w, b, tc.CNL_RELU, residual=res, algo=tc.CNL_ALGO_FORCE + variant, want=5, ymax=True)
    assert bool(torch.isfinite(want).all())
    for kind in ("nan", "inf", "mix", "border"):
        if kind == "border":
            bx, br = x.clone(), res.clone()
            for t in (bx, br):
                t[1, :, 0], t[1, :, -1], t[1, :, :, 0], t[1, :, :, -1] = INF, INF, INF, INF
        else:
            bx, br = _poison(x, kind, 1), _poison(res, kind, 2)
        got, gm = tc.run_winograd(bx, w, b, tc.CNL_RELU, residual=br, algo=tc.CNL_ALGO_FORCE + variant, want=5, ymax=True)
        for n in (0, 2):
            assert _same_bits(got[n], want[n]) and _same_bits(gm[n], wm[n]), (kind, n)


# ============================================================================================================================ part B: behind the network
POISONS = ("nan", "inf", "-inf", "mix")


def _poison(t, kind, seed):
    """A copy of t (batch first) with item 1 replaced by the pattern."""
    t = t.clone()
    if kind == "mix":
        g = torch.Generator().manual_seed(seed)
        table = torch.tensor([NAN, INF, -INF, HUGE, -HUGE])
        t[1] = table[torch.randint(0, 5, tuple(t[1].shape), generator=g)]
    else:
        t[1] = {"nan": NAN, "inf": INF, "-inf": -INF}[kind]
    return t


def _others_keep_their_bits(got, want, what):
    for key in want:
        for n in (0, 2):
            assert _same_bits(got[key][n], want[key][n]) if got[key].dtype == torch.float32 else torch.equal(got[key][n], want[key][n]), (what, key, n)


# ---------------------------------------------------------------------------------------------------------------------------- cnl_decode_f32
# (name, C, H, W, k, E, layout, stage-1 form, top-k key storage): one shape per stage-1 kernel (1 channel-minor, 2 channel-minor C % 8 == 0, 3 class planes,
# 4 generic) and per key storage (0 sixteen registers, 1 LDS, 2 forty-eight registers, 3 upper halves in LDS, 4 memory), the smallest of
# tests/test_gpu_decode.py's shapes that take them; every case also runs in the other layout (which takes another stage-1 kernel)
DECODE = [("generic_regs16", 16, 33, 47, 40, 4, "nchw", 4, 0), ("planes_regs16", 4, 16, 132, 64, 0, "nchw", 3, 0), ("cminor_regs16", 5, 33, 47, 40, 0, "nhwc", 1, 0),
          ("c8_regs16", 16, 128, 128, 100, 0, "nhwc", 2, 0), ("c8_lds32", 8, 150, 150, 100, 0, "nhwc", 2, 1), ("planes_regs48", 4, 152, 272, 300, 8, "nchw", 3, 2),
          ("cminor_lds16", 2, 199, 201, 100, 0, "nhwc", 1, 3), ("c8_memory", 8, 224, 224, 100, 0, "nhwc", 2, 4)]


def _as(t, layout):
    """A logical-NCHW device tensor whose memory is NCHW or NHWC."""
    t = t.cuda()
    return t.contiguous() if layout == "nchw" else t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _decode(heat, box, reid, k, fill):
    """One cnl_decode_f32 launch into outputs pre-filled with `fill` -> (outputs, (stage1, vec, strip, topk))."""
    lib = _lib.load()
    N, C, H, W = heat.shape
    E = reid.shape[1] if reid is not None else 0
    out = {"scores": torch.full((N, k), float(fill), device="cuda"), "indices": torch.full((N, k), int(fill), device="cuda", dtype=torch.int64),
           "labels": torch.full((N, k), int(fill), device="cuda", dtype=torch.int64), "boxes": torch.full((N, k, 4), float(fill), device="cuda")}
    if E:
        out["emb"] = torch.full((N, k, E), float(fill), device="cuda")
    ws_bytes = int(lib.cnl_decode_workspace_bytes(N, H, W))
    ws = torch.empty((ws_bytes,), device="cuda", dtype=torch.uint8)
    p = _lib.DecodeParams()
    p.heat, p.box = heat.data_ptr(), box.data_ptr()
    p.heat_sn, p.heat_sc, p.heat_sh, p.heat_sw = heat.stride()
    p.box_sn, p.box_sc, p.box_sh, p.box_sw = box.stride()
    if E:
        p.reid, p.emb = reid.data_ptr(), out["emb"].data_ptr()
        p.reid_sn, p.reid_sc, p.reid_sh, p.reid_sw = reid.stride()
    p.N, p.C, p.H, p.W, p.E, p.k, p.nms_kernel = N, C, H, W, E, k, 3
    p.normalize_boxes, p.box_log, p.box_multiplier, p.stride = 0, 0, 1.0, 4.0
    p.scores, p.indices, p.labels, p.boxes = (out[key].data_ptr() for key in ("scores", "indices", "labels", "boxes"))
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws_bytes
    forms = [ctypes.c_int32(-1) for _ in range(4)]
    _lib.check(lib.cnl_decode_forms(ctypes.byref(p), *(ctypes.byref(f) for f in forms)), "cnl_decode_forms")
    _lib.check(lib.cnl_decode_f32(ctypes.byref(p), _stream()), "cnl_decode_f32")
    torch.cuda.synchronize()
    return out, tuple(f.value for f in forms)


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("case", DECODE, ids=[c[0] for c in DECODE])
def test_decode_of_a_non_finite_image_keeps_the_others_and_stays_in_range(case, poison):
    """heat, box and reid of image 1 of 3 are non-finite.  Images 0 and 2 keep the bits of scores, indices, labels, boxes and embeddings; image 1's indices lie
    in [0, H W) and are pairwise distinct and its labels lie in [0, C) — what keeps the gathers and crops behind the decode inside their buffers; every output
    element is written (outputs pre-filled with 1 and with 2: an element that holds its pre-fill both times was not written); the forms are the ones the case
    is there for; the same data in the other layout (another stage-1 kernel) keeps images 0 and 2 as well.

    The poisoned image itself across layouts, measured on the MI355X: the same bytes from the NCHW and the NHWC launch in all 8 shapes for an all-NaN, an
    all +Inf and an all -Inf image; with the mix, different bytes in 5 of the 8 (generic against c8 at C = 16, planes against channel-minor at C = 4, c8
    against planes at C = 8 and 16).  Every stage-1 kernel gives a thread its own subset of the classes, takes the subset's first class unconditionally and a later one only if it
    compares greater — never, with a NaN on either side — and merges the subsets by another float compare or by the integer score key, so WHICH NaN of a
    pixel survives depends on the kernel.  The header's "every combination computes the same bytes" is therefore stated for finite heat values; the poisoned image is not compared.

    Why topk_kernel terminates whatever the keys (read before the first run): score_key maps EVERY bit pattern, NaN included, to an unsigned integer, and from
    there on the kernel compares integers only.  Phase A and the compaction loop over H W and over the at most 64 bits of a per-thread mask (each round
    clears one bit of every lane that still has one, so the `for (;;)` ends after at most 64 rounds); the bound's second step is one histogram of the 1024
    thread maxima in (range >> bsh) < 1024 bins with bsh = 22 - clz(range) — range up to 2^32 - 1 gives bsh = 22 — scanned once by one wave; the rank step
    loops over the candidate count (<= 1024); the radix select is three passes of fixed digit widths (12 / 10 / 10 bits) over H W keys and 4096 / 1024 bins.
    No trip count depends on a key's value, only on H W, k and counts of keys."""
    name, C, H, W, k, E, layout, s1, tk = case
    g = torch.Generator().manual_seed(C * 1000 + H + W)
    heat = torch.rand(3, C, H, W, generator=g)
    box = torch.rand(3, 4, H, W, generator=g) * 7 - 0.5
    reid = torch.randn(3, E, H, W, generator=g) if E else None
    bad = [_poison(t, poison, 7 + j) if t is not None else None for j, t in enumerate((heat, box, reid))]
    other = "nhwc" if layout == "nchw" else "nchw"
    clean, forms = _decode(*(_as(t, layout) if t is not None else None for t in (heat, box, reid)), k, 1.0)
    assert (forms[0], forms[3]) == (s1, tk), forms
    for lay in (layout, other):
        dev = [_as(t, lay) if t is not None else None for t in bad]
        o1, f1 = _decode(*dev, k, 1.0)
        o2, _ = _decode(*dev, k, 2.0)
        assert lay != layout or f1 == forms, (f1, forms)
        _others_keep_their_bits(o1, clean, (name, poison, lay))
        _others_keep_their_bits(o2, clean, (name, poison, lay))
        idx, lab = o1["indices"][1], o1["labels"][1]
        assert bool(((idx >= 0) & (idx < H * W)).all()) and idx.unique().numel() == k, (name, poison, lay, "indices of the poisoned image")
        assert bool(((lab >= 0) & (lab < C)).all()), (name, poison, lay, "labels of the poisoned image")
        for key in o1:
            unwritten = (o1[key] == 1) & (o2[key] == 2)
            assert not bool(unwritten.any()), (name, poison, lay, key, int(unwritten.sum()))


def test_gathers_of_a_non_finite_image_keep_the_others():
    """cnl_gather_boxes_f32 / cnl_gather_embeddings_f32 at valid indices, box and reid of image 1 non-finite: the rows of images 0 and 2 keep their bits; the
    embedding gather is a copy, so image 1's rows are the map's own bits."""
    N, H, W, k, E = 3, 11, 14, 40, 6
    g = torch.Generator().manual_seed(5)
    box, reid = torch.rand(N, 4, H, W, generator=g) * 7 - 0.5, torch.randn(N, E, H, W, generator=g)
    idx = torch.stack([torch.randperm(H * W, generator=g)[:k] for _ in range(N)]).cuda()
    for layout in ("nchw", "nhwc"):
        want = {"boxes": cl.decode.gather_boxes(_as(box, layout), idx), "emb": cl.decode.gather_embeddings(_as(reid, layout), idx)}
        for poison in POISONS:
            bad_reid = _as(_poison(reid, poison, 3), layout)
            got = {"boxes": cl.decode.gather_boxes(_as(_poison(box, poison, 2), layout), idx), "emb": cl.decode.gather_embeddings(bad_reid, idx)}
            _others_keep_their_bits(got, want, ("gathers", layout, poison))
            copy = bad_reid[1].flatten(1)[:, idx[1]].t()
            assert _same_bits(got["emb"][1], copy), (layout, poison)


@pytest.mark.parametrize("E", [0, 5])
def test_pack_and_unpack_of_a_non_finite_image_keep_the_others(E):
    """cnl_pack_detections_f32 / cnl_unpack_detections_f32 move bits: the records of images 0 and 2 are those of the clean batch, and unpacking returns every
    image's input bits, the poisoned one's included."""
    N, k = 3, 37
    g = torch.Generator().manual_seed(E)
    dets = {"bboxes": torch.rand(N, k, 4, generator=g) * 100, "scores": torch.rand(N, k, generator=g), "labels": torch.randint(0, 80, (N, k), generator=g)}
    if E:
        dets["embeddings"] = torch.randn(N, k, E, generator=g)
    want = cl.collate.pack_detections({key: v.cuda() for key, v in dets.items()})
    for poison in POISONS:
        bad = {key: (_poison(v, poison, 11) if v.dtype == torch.float32 else v).cuda() for key, v in dets.items()}
        rec = cl.collate.pack_detections(bad)
        assert _same_bits(rec[0], want[0]) and _same_bits(rec[2], want[2]), poison
        back = cl.collate.unpack_detections(rec)
        for key, v in bad.items():
            assert _same_bits(back[key], v) if v.dtype == torch.float32 else torch.equal(back[key], v), (poison, key)


def test_flip_merge_of_a_non_finite_image_keeps_the_others():
    """cnl_flip_merge_f32, image 1 non-finite in the plain half, in the mirrored half, and in both: merged images 0 and 2 keep their bits; image 1 is what the
    header says — one IEEE add and one multiply by 0.5, NaN and Inf propagating as they fall: NaN exactly where (a + b.flip(-1)[:, perm]) * 0.5 is NaN, the
    bits of that expression everywhere else."""
    N, H, W = 3, 12, 20
    g = torch.Generator().manual_seed(9)
    maps = OrderedDict([("heatmap", torch.rand(2 * N, 8, H, W, generator=g)), ("box_2d", torch.rand(2 * N, 4, H, W, generator=g) * 9), ("reid", torch.randn(2 * N, 5, H, W, generator=g))])
    for layout in ("nchw", "nhwc"):
        want = cl.flip.flip_merge(OrderedDict((key, _as(v, layout)) for key, v in maps.items()), N)
        for poison in POISONS:
            for halves in ((1,), (N + 1,), (1, N + 1)):
                bad = OrderedDict()
                for j, (key, v) in enumerate(maps.items()):
                    v = v.clone()
                    for h in halves:
                        v[h] = _poison(v[h - 1:h + 2], poison, 20 + j)[1]
                    bad[key] = _as(v, layout)
                got = cl.flip.flip_merge(bad, N)
                torch.cuda.synchronize()
                _others_keep_their_bits(got, want, ("flip merge", layout, poison, halves))
                for key, v in bad.items():
                    b = v[N:].flip(-1)
                    if key == "box_2d":
                        b = b[:, [2, 1, 0, 3]]
                    ieee = (v[:N] + b) * 0.5
                    nan = torch.isnan(ieee)
                    assert torch.equal(torch.isnan(got[key]), nan) and _same_bits(torch.where(nan, 0.0, got[key]), torch.where(nan, 0.0, ieee)), (key, layout, poison, halves)
                    assert bool(nan[1].any()) or poison in ("inf", "-inf")              # (the poison reached the merged image)


def test_unletterbox_of_a_non_finite_frame_keeps_the_others():
    """cnl_unletterbox_boxes_f32, the boxes of frame 1 non-finite: frames 0 and 2 keep their bits, clipped or not."""
    g = torch.Generator().manual_seed(3)
    frames = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).cuda() for (h, w) in ((40, 60), (64, 48), (33, 50))]
    _, geom = cl.letterbox.letterbox_uint8(frames, 64, 64)
    boxes = torch.rand(3, 29, 4, generator=g) * 70 - 3
    for clip in (True, False):
        want = cl.letterbox.unletterbox(boxes.cuda(), geom, clip=clip)
        for poison in POISONS:
            got = cl.letterbox.unletterbox(_poison(boxes, poison, 4).cuda(), geom, clip=clip)
            _others_keep_their_bits({"boxes": got}, {"boxes": want}, ("unletterbox", clip, poison))


def test_tile_merge_of_a_non_finite_frame_keeps_the_others():
    """cnl_merge_tiles_f32 on three frames of two views each, the candidates of frame 1 non-finite: frames 0 and 2 keep every output (boxes, scores, labels,
    source, count).  Frame 1 as the header defines it: a NaN score never takes part — all scores NaN gives count 0 and rows of score 0, label 0, box 0,
    source -1; a NaN coordinate becomes 0 — with finite scores and non-finite boxes no NaN reaches the output and every kept box lies in [0, frame_w] x
    [0, frame_h]; every output element is written."""
    N, k, K = 3, 16, 24
    fw, fh = 96, 80
    records = [(fw, fh, x0, 0, 0, 0, 1.0, 1.0) for _ in range(N) for x0 in (0, 32)]
    geom = cl.tiles.TileGeometry.from_records(records, [0, 2, 4, 6], "cuda")
    g = torch.Generator().manual_seed(14)
    xy = torch.rand(2 * N, k, 2, generator=g) * 40
    boxes = torch.cat([xy, xy + 4 + torch.rand(2 * N, k, 2, generator=g) * 20], -1)
    scores = torch.rand(2 * N, k, generator=g) * 0.9 + 0.1
    labels = torch.randint(0, 3, (2 * N, k), generator=g)
    merge = lambda b, s: cl.tiles.merge_tiles(b.cuda(), s.cuda(), labels.cuda(), geom, max_detections=K, score_threshold=0.05)
    want = merge(boxes, scores)
    assert int(want["count"].min()) > 0

    def frame1(t, kind, seed):                  # views 2 and 3 are frame 1's
        t = t.clone()
        t[2:4] = _poison(torch.stack([t[2:4]] * 3), kind, seed)[1]
        return t

    for poison in POISONS:
        for what in ("scores", "boxes", "both"):
            b = frame1(boxes, poison, 1) if what != "scores" else boxes
            s = frame1(scores, poison, 2) if what != "boxes" else scores
            got = merge(b, s)
            torch.cuda.synchronize()
            _others_keep_their_bits(got, want, ("tile merge", poison, what))
            c = int(got["count"][1])
            assert 0 <= c <= K and not bool(torch.isnan(got["bboxes"][1]).any()), (poison, what, c)
            assert bool((got["bboxes"][1, :, 0::2] >= 0).all() and (got["bboxes"][1, :, 0::2] <= fw).all() and (got["bboxes"][1, :, 1::2] >= 0).all()
                        and (got["bboxes"][1, :, 1::2] <= fh).all()), (poison, what)
            assert bool((got["source"][1, :c] >= 0).all() and (got["source"][1, :c] < 2 * k).all() and (got["source"][1, c:] == -1).all()), (poison, what)
            assert bool((got["scores"][1, c:] == 0).all() and (got["labels"][1, c:] == 0).all() and (got["bboxes"][1, c:] == 0).all()), (poison, what)
            if poison == "nan" and what != "boxes":
                assert c == 0, (what, c)
