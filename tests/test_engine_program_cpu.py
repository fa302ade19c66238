"""CPU: the engine's launch programs, compared against tests/golden/engine_programs.json.

The engine (adaptsegnet_amd/engine.py) is host code that turns a model into a fixed program of
native launches.  With the op table (kernels._OP) replaced by a recorder it runs on untouched CPU
``torch.empty`` tensors: the planning queries it asks are host arithmetic.  A trace holds, per op
call in order, the op's name and every argument: numbers, bools, None and lists as they are, a
tensor as dtype, shape, strides ("c": contiguous) and an identity number that is unique within the
trace, so aliasing (in-place BN backward, ``out=gout, res=gout``) and the data flow between calls
are pinned as well.  A changed launch, argument, alias or order shows here as a diff that names the
case, the op and the argument, before (or without) any number moving on the GPU.

Fixture layout (data only, every level stored once): ``args`` holds the distinct argument texts, a
tensor's identity number replaced by ``#``; a ``lines`` entry is an op name and its arguments as
indices into ``args``; an ``ops`` entry is a line index and that call's tensors, each written
relative to the list of live tensors (first seen, not yet used for the last time, oldest first):
``n`` a tensor first seen here, ``x`` one first seen here and never again, ``k`` the k-th live tensor
from the newest, ``-k`` the same at its last use; so the calls of equal blocks are equal entries.  A
``programs`` entry lists op indices, ``( a b c )*22`` standing for 22 repeats; ``block_cases`` gives, per maths and switch setting, the
programs of that group's cases in the order block_cases() names them, and ``cases`` maps the
whole-model case names to theirs.  decode() turns it back into the traces' own form, so a failure
prints both op lines in full.  The fixture was recorded from the engine.py / kernels.py of commit
RECORDED_AT.

Running this module as a script rewrites the fixture:  python tests/test_engine_program_cpu.py
"""
import json
import os
import sys
import time

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_programs.json")
RECORDED_AT = "5d53f5f"   # the commit whose engine.py / kernels.py produced the fixture

# (inplanes, planes, stride, dilation, downsample)
BLOCKS = [(64, 64, 1, 1, True), (256, 64, 1, 1, False), (256, 128, 2, 1, True), (512, 128, 1, 1, False),
          (512, 256, 1, 2, True), (1024, 256, 1, 2, False), (1024, 512, 1, 4, True), (2048, 512, 1, 4, False)]
MATHS = ("MATH_F32", "MATH_BF16", "MATH_F32X3", "MATH_F32X3_PRESPLIT")
# interior block with every fp32 form / interior block with none / first block (fp32 x, no copy)
SITUATIONS = ("interior", "interior_low", "first")
# engine switch settings, one at a time against the defaults
SETTINGS = {"defaults": {}}
SETTINGS.update({f"fwd_terms1_bwd{b}": {"X3_FWD_TERMS": 1, "X3_BWD_TERMS": b} for b in (0, 1, 2, 3)})
SETTINGS.update({f"wgrad_min_c{c}": {"X3_WGRAD_TERMS_MIN_C": c} for c in (0, 256)})
SETTINGS.update({"mask_bits0": {"MASK_BITS": 0}, "bf16_grads0": {"BF16_GRADS": 0}})
SETTINGS.update({f"bn_fold{v}": {"BN_FOLD": v} for v in (1, 2, 3)})
SETTINGS.update({f"bn_sums{v}": {"BN_SUMS": v} for v in (1, 2, 3)})
# below this size the plans of the two dilated identity blocks cannot fuse BN_FOLD / BN_SUMS
BIG = (65, 129)
BIG_BLOCKS = (BLOCKS[5], BLOCKS[7])
BIG_SETTINGS = ("defaults", "bn_fold1", "bn_fold2", "bn_fold3", "bn_sums1", "bn_sums2", "bn_sums3")

# ops of ops.NAMES that no trace holds, with the reason
NOT_TRACED = {name: "not launched by engine.py (losses, optimisers, data pipeline, evaluation, pseudo-labels)"
              for name in ("softmax_fwd", "softmax_bwd", "softmax_ce_fwd", "softmax_ce_bwd", "adv_loss_fwd",
                           "adv_loss_bwd", "sgd_step", "adam_step", "axpy", "gta5_preprocess",
                           "gta5_preprocess_augment", "upsample_argmax", "fuse_argmax", "confusion_hist",
                           "conf_hist", "pseudo_thresholds", "pseudo_label")}

_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32", torch.int64: "i64", torch.uint8: "u8"}


class Recorder:
    """Stands in for kernels._OP: every attribute is an op that records its call."""

    def __init__(self):
        self.begin()

    def begin(self):
        self.calls, self.ids, self.keep = [], {}, []

    def __getattr__(self, name):
        def op(*args):
            ids = []
            self.calls.append((f"{name}({', '.join(self._arg(a, ids) for a in args)})", ids))
        return op

    def _arg(self, a, ids):
        if isinstance(a, torch.Tensor):
            # (every tensor seen stays referenced until the trace ends: no address is reused)
            self.keep.append(a)
            key = a.data_ptr() if a.numel() else ("empty", id(a))
            ids.append(self.ids.setdefault(key, len(self.ids)))
            strides = "c" if a.is_contiguous() else "s" + ",".join(str(s) for s in a.stride())
            return f"{_DT[a.dtype]}[{','.join(str(s) for s in a.shape)}]{strides}#"
        if isinstance(a, (list, tuple)):
            return "[" + ", ".join(self._arg(v, ids) for v in a) + "]"
        assert a is None or isinstance(a, (bool, int, float)), type(a)
        return repr(a)


def render(call):
    """An op line with its identity numbers filled in (for failure messages)."""
    line, ids = call
    parts = line.split("#")
    return "".join(p + (f"#{ids[i]}" if i < len(ids) else "") for i, p in enumerate(parts))


def block_cases(math, sname):
    """[(case name, block, training, situation, (h, w))] of one maths and switch setting, in order."""
    out = []
    for spec in BLOCKS:
        sizes = [(9, 11)]
        if math == "MATH_F32X3" and spec in BIG_BLOCKS and sname in BIG_SETTINGS:
            sizes.append(BIG)
        for hw in sizes:
            for training in (True, False):
                for sit in SITUATIONS:
                    name = (f"block {spec[0]}-{spec[1]} s{spec[2]} d{spec[3]} ds{int(spec[4])} "
                            f"{hw[0]}x{hw[1]} {math} {'train' if training else 'eval'} {sit} {sname}")
                    out.append((name, spec, training, sit, hw))
    return out


def _empty(shape, dtype=torch.float32, channels_last=False):
    t = torch.empty(shape, dtype=dtype)
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t


class Tracer:
    """Runs engine programs on the CPU with the stubs the issue of this test lists: the op table a
    recorder, kernels._require a no-op, engine.WGRAD_STREAM 0."""

    def __init__(self, mp):
        from adaptsegnet_amd import engine, kernels
        self.E, self.K, self.mp = engine, kernels, mp
        self.rec = Recorder()
        mp.setattr(kernels, "_OP", self.rec)
        mp.setattr(kernels, "_require", lambda t, what: None)
        mp.setattr(engine, "WGRAD_STREAM", 0)
        self.cpu = torch.device("cpu")
        self._blocks = {}
        self.traces = {}

    def trace(self, name, fn):
        self.rec.begin()
        fn()
        assert name not in self.traces, name
        self.traces[name] = self.rec.calls
        self.rec.begin()

    # -- one Bottleneck: block_forward(save=True) then block_backward(need_w=True, ws=None) -------
    def block(self, spec):
        blk = self._blocks.get(spec)
        if blk is None:
            from adaptsegnet_amd.model.deeplab_multi import Bottleneck
            from adaptsegnet_amd.model.layers import BatchNorm2d, Conv2d
            cin, planes, stride, dil, ds = spec
            down = None
            if ds:
                down = torch.nn.Sequential(Conv2d(cin, planes * 4, kernel_size=1, stride=stride, bias=False),
                                           BatchNorm2d(planes * 4))
            blk = self._blocks[spec] = Bottleneck(cin, planes, stride, dilation=dil, downsample=down)
            for m in blk.modules():
                if isinstance(m, Conv2d):
                    m.weight.grad = torch.empty_like(m.weight)
        return blk

    def run_block(self, spec, training, situation, hw, n=2):
        E, K = self.E, self.K
        blk = self.block(spec)
        h, w = hw
        x, xb = _empty((n, h, w, spec[0])), None
        if situation != "first" and E.bf16_operands():
            xb = K._bf16_like(x, True)
            if E.lowp_storage() and not E.block_input_fp32(blk, n, h, w):
                x = None   # bf16 activation storage: the producer wrote no fp32 output
        full = situation != "interior_low"
        out, rec, outb = E.block_forward(blk, x, n, h, w, training, True, xb=xb, out_fp32=full)
        oh, ow = blk.conv1.geom().out_hw(h, w)
        low = E.lowp_grads() and situation != "interior"
        gout = _empty((n, oh, ow, 4 * spec[1]), torch.bfloat16 if low else torch.float32)
        E.block_backward(blk, rec, gout, True, None, dx_fp32=full)

    def block_cases(self):
        K = self.K
        for math in MATHS:
            K.set_conv_math(getattr(K, math))
            for sname, setting in SETTINGS.items():
                with self.mp.context() as m:
                    for k, v in setting.items():
                        m.setattr(self.E, k, v)
                    for name, spec, training, sit, hw in block_cases(math, sname):
                        self.trace(name, lambda: self.run_block(spec, training, sit, hw))

    # -- whole programs ----------------------------------------------------------------------
    def _fresh(self, model):
        model._ensure_arena(self.cpu)
        model._arena.zero_grad()
        return model._anchors[True]

    def deeplab_cases(self):
        from adaptsegnet_amd.model import DeeplabMulti
        K, E = self.K, self.E
        model = DeeplabMulti(num_classes=19)
        for math in MATHS:
            K.set_conv_math(getattr(K, math))
            for training in (True, False):
                for first_head in (True, False):
                    model.train(training)
                    anchor = self._fresh(model)

                    def run():
                        x = _empty((2, 3, 41, 57))
                        y1, y2 = E._DeeplabMultiFn.apply(anchor, x, model, 41, 57, True, first_head)
                        outs = [y for y in (y1, y2) if y is not None]
                        torch.autograd.backward(outs, [_empty(y.shape, channels_last=True) for y in outs])
                    self.trace(f"DeeplabMulti 2x3x41x57 {math} {'train' if training else 'eval'} "
                               f"first_head{int(first_head)}", run)

    def discriminator_cases(self):
        from adaptsegnet_amd.model import FCDiscriminator
        K, E = self.K, self.E
        model = FCDiscriminator(num_classes=19)
        for math in ("MATH_F32X3", "MATH_BF16"):
            K.set_conv_math(getattr(K, math))
            anchor = self._fresh(model)
            keep = E.DiscForward()

            def run():
                x = _empty((2, 19, 41, 57), channels_last=True).requires_grad_()
                with K.weight_pack_scope():   # (the trainer's scope: the weight packs are launches too)
                    y = E._FCDiscriminatorFn.apply(anchor, x, model, True, keep)
                    y.backward(_empty(y.shape, channels_last=True))
            self.trace(f"FCDiscriminator keep 2x19x41x57 {math}", run)

            def replay():
                y = E._DiscReplayFn.apply(anchor, model, keep)
                y.backward(_empty(y.shape, channels_last=True))
            self.trace(f"DiscReplay 2x19x41x57 {math}", replay)
        K.clear_weight_packs()

    def vgg_cases(self):
        from adaptsegnet_amd.model.deeplab_vgg import DeeplabVGG
        K, E = self.K, self.E
        model = DeeplabVGG(num_classes=19)
        K.set_conv_math(K.MATH_F32X3)
        for terms in (0, 1, 2):
            with self.mp.context() as m:
                m.setattr(E, "VGG_TERMS", terms)
                m.setattr(E, "VGG_TERMS_MIN_C", 256)   # (the term path at this model's 256 / 512 / 1024 widths)
                anchor = self._fresh(model)

                def run():
                    y = E._DeeplabVGGFn.apply(anchor, _empty((2, 3, 41, 57)), model, True)
                    y.backward(_empty(y.shape))   # (an NCHW gradient: the engine copies it to NHWC)
                self.trace(f"DeeplabVGG 2x3x41x57 MATH_F32X3 vgg_terms{terms}", run)

    def warper_case(self):
        from adaptsegnet_amd.model.warper import Warper
        K, E = self.K, self.E
        model = Warper().train()
        K.set_conv_math(K.MATH_F32X3)
        anchor = self._fresh(model)

        def run():   # 256: the smallest side the eight-level encoder's divisibility check accepts
            outs = E._WarperFn.apply(anchor, _empty((1, 3, 256, 256)), model, True)
            outs[0].backward(_empty(outs[0].shape, channels_last=True))
        self.trace("Warper 1x3x256x256 MATH_F32X3 train", run)

    def warp_case(self):
        E = self.E

        def run():
            flow = _empty((2, 2, 9, 11)).requires_grad_()
            x1, x2 = (_empty((2, 19, 9, 11), channels_last=True).requires_grad_() for _ in range(2))
            y1, y2 = E._GridWarpFn.apply(flow, x1, x2)
            torch.autograd.backward([y1, y2], [_empty(y1.shape), _empty(y2.shape, channels_last=True)])
        self.trace("grid_warp 2x19x9x11", run)


def build_traces():
    """{case name: [(op line, identity numbers)]} of every case, and the seconds it took."""
    from adaptsegnet_amd import kernels as K
    t0 = time.perf_counter()
    saved = K.get_conv_math()
    with pytest.MonkeyPatch.context() as mp:
        try:
            tr = Tracer(mp)
            tr.block_cases()
            tr.deeplab_cases()
            tr.discriminator_cases()
            tr.vgg_cases()
            tr.warper_case()
            tr.warp_case()
        finally:
            K.set_conv_math(saved)
    return tr.traces, time.perf_counter() - t0


def _split_args(line):
    """(op name, [argument texts]) of an op line: split at each ", " outside a list."""
    name, rest = line[:-1].split("(", 1)
    args, depth = [""], 0
    for part in rest.split(", "):
        args[-1] += part
        depth += part.count("[") - part.count("]")
        if depth == 0:
            args.append("")
        else:
            args[-1] += ", "
    return name, args[:-1]


def _index(table, key):
    return table.setdefault(key, len(table))


def _pack(seq):
    """A list of tokens as text, a run repeated r times in a row written once as ``( ... )*r``."""
    out, i = [], 0
    while i < len(seq):
        best = (0, 1, 1)
        for p in range(1, 61):
            r = 1
            while seq[i + r * p:i + (r + 1) * p] == seq[i:i + p]:
                r += 1
            best = max(best, ((r - 1) * p, p, r))
        saved, p, r = best
        out += ["("] + seq[i:i + p] + [f")*{r}"] if saved > 2 else seq[i:i + 1]
        i += p * r if saved > 2 else 1
    return " ".join(out)


def _unpack(text):
    out, start = [], None
    for tok in text.split():
        if tok == "(":
            start = len(out)
        elif tok.startswith(")*"):
            out += out[start:] * (int(tok[2:]) - 1)
        else:
            out.append(tok)
    return out


def encode(traces):
    """The fixture's content (see the module docstring)."""
    args, lines, ops, programs, cases = {}, {}, {}, {}, {}
    for name, calls in traces.items():
        last = {i: (c, k) for c, (_, ids) in enumerate(calls) for k, i in enumerate(ids)}   # each tensor's last use
        prog, live, seen = [], [], 0
        for c, (line, ids) in enumerate(calls):
            op, texts = _split_args(line)
            rel = []
            for k, i in enumerate(ids):
                dead = last[i] == (c, k)
                if i == seen:
                    seen += 1
                    rel.append("x" if dead else "n")
                    live += [] if dead else [i]
                else:
                    at = len(live) - live.index(i)
                    rel.append(f"-{at}" if dead else str(at))
                    if dead:
                        live.remove(i)
            li = _index(lines, " ".join([op] + [str(_index(args, t)) for t in texts]))
            prog.append(str(_index(ops, " ".join([str(li)] + rel))))
        cases[name] = _index(programs, _pack(prog))
    groups = {f"{m} {sn}": " ".join(str(cases.pop(c[0])) for c in block_cases(m, sn)) for m in MATHS for sn in SETTINGS}
    return {"recorded_at": RECORDED_AT, "args": list(args), "lines": list(lines), "ops": list(ops),
            "programs": list(programs), "block_cases": groups, "cases": cases}


def decode(data):
    """{case name: [(op line, identity numbers)]} of a fixture: what build_traces() returns."""
    lines = []
    for entry in data["lines"]:
        op, *idx = entry.split()
        lines.append(f"{op}({', '.join(data['args'][int(i)] for i in idx)})")
    programs = []
    for entry in data["programs"]:
        calls, live, seen = [], [], 0
        for o in _unpack(entry):
            li, *rel = data["ops"][int(o)].split()
            ids = []
            for r in rel:
                if r in "nx":
                    ids.append(seen)
                    live += [seen] if r == "n" else []
                    seen += 1
                else:
                    ids.append(live[-abs(int(r))])
                    if r[0] == "-":
                        live.remove(ids[-1])
            calls.append((lines[int(li)], ids))
        programs.append(calls)
    cases = {name: programs[i] for name, i in data["cases"].items()}
    for group, entry in data["block_cases"].items():
        math, sname = group.split()
        names = [c[0] for c in block_cases(math, sname)]
        idx = entry.split()
        assert len(names) == len(idx), group
        cases.update({name: programs[int(i)] for name, i in zip(names, idx)})
    return cases


def write_fixture(data):
    def rows(key, per_line=1):
        v = data[key]
        packed = [v[i:i + per_line] for i in range(0, len(v), per_line)]
        return f'"{key}": [\n' + ",\n".join(json.dumps(r, separators=(",", ":"))[1:-1] for r in packed) + "\n]"

    def table(key):
        return f'"{key}": {{\n' + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in data[key].items()) + "\n}"
    with open(FIXTURE, "w") as f:
        f.write('{\n"recorded_at": ' + json.dumps(data["recorded_at"]) + ",\n" + ",\n".join(
            [rows("args", 4), rows("lines", 2), rows("ops", 8), rows("programs"), table("block_cases"), table("cases")])
            + "\n}\n")


@pytest.fixture(scope="module")
def traced():
    return build_traces()


def test_programs_match_the_fixture(traced):
    traces = traced[0]
    with open(FIXTURE) as f:
        want = decode(json.load(f))
    assert sorted(traces) == sorted(want), set(traces) ^ set(want)
    bad = []
    for name, calls in traces.items():
        rec = want[name]
        if rec != [(line, ids) for line, ids in calls]:
            i = next((i for i, (a, b) in enumerate(zip(calls, rec)) if (a[0], a[1]) != b), min(len(calls), len(rec)))
            now = render(calls[i]) if i < len(calls) else "(program ends)"
            then = render(rec[i]) if i < len(rec) else "(program ends)"
            bad.append(f"{name}: op {i} of {len(calls)} (recorded: {len(rec)})\n  now:      {now}\n  recorded: {then}")
    assert not bad, f"{len(bad)} of {len(traces)} programs differ; first:\n" + bad[0]


def test_every_switch_setting_changes_a_program(traced):
    """Each listed setting changes at least one traced block program relative to the defaults."""
    traces = traced[0]
    for sname in SETTINGS:
        if sname == "defaults":
            continue
        mine = [n for n in traces if n.startswith("block ") and n.endswith(" " + sname)]
        assert mine, sname
        assert any(traces[n] != traces[n[:-len(sname)] + "defaults"] for n in mine), sname
    vgg = [traces[f"DeeplabVGG 2x3x41x57 MATH_F32X3 vgg_terms{t}"] for t in (0, 1, 2)]
    assert vgg[0] != vgg[1] and vgg[1] != vgg[2] and vgg[0] != vgg[2]


def test_every_engine_op_is_traced(traced):
    """Every op of ops.NAMES appears in some trace, or is listed in NOT_TRACED with the reason."""
    from adaptsegnet_amd import ops
    seen = {line.split("(", 1)[0] for calls in traced[0].values() for line, _ in calls}
    assert seen <= set(ops.NAMES), seen - set(ops.NAMES)
    assert set(ops.NAMES) - seen == set(NOT_TRACED), (set(ops.NAMES) - seen) ^ set(NOT_TRACED)


def test_tracing_stays_quick(traced):
    assert traced[1] < 120, f"tracing took {traced[1]:.0f} s"


if __name__ == "__main__":
    trs, secs = build_traces()
    data = encode(trs)
    write_fixture(data)
    with open(FIXTURE) as f:
        assert decode(json.load(f)) == {k: [(line, ids) for line, ids in v] for k, v in trs.items()}
    print(f"{len(trs)} cases, {len(data['programs'])} programs, {len(data['ops'])} ops, {len(data['lines'])} lines, "
          f"{len(data['args'])} args, {secs:.0f} s, {os.path.getsize(FIXTURE)} bytes")
