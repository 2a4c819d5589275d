"""conv_plan (csrc/conv_igemm.hip): the one function that says which kernel serves a conv descriptor, with which packed-weight layout
and which GroupNorm partial rows.  tests/golden/conv_plan_table.json records its answers — and those of the two queries that read it,
vq_conv_weight_layout and vq_conv2d_gn_tile — for the model's layers and the shapes that reach every instantiation, under every hint the
kernel tests use.  The plan is read through vq_debug_conv_plan, which only `make ABLATE=1` / emulator builds carry: CPU only.

Re-record after a deliberate change of the selection:  python tests/test_conv_plan.py --record
"""
import ctypes as C
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "conv_plan_table.json")
SOURCE = os.path.join(ROOT, "vqgan-training_amd", "csrc", "conv_igemm.hip")
BF16, F32, F16, F16X2 = 0, 1, 2, 3
DESC = ("N", "H", "W", "Cin", "Ho", "Wo", "Cout", "R", "stride", "dil_in", "up", "pad", "subpix", "dtype", "split")
PLAN = ("family", "BC", "BP", "WC", "WP", "v0", "v1", "v2", "layout", "gn_bp", "gn_nw", "gn_row")
GROUPS = 32
# every kernel_hint the kernel tests pass (test_kernels.py, test_tap9_wide.py), and the A/B knobs of include/vqhip.h
HINTS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 3 + (512 << 4), 5 + (72 << 4), 5 + (128 << 4), 5 + (256 << 4), 1 + (32 << 4), 16 << 4, 40 << 4,
         48 << 4, 56 << 4, 5 + (80 << 4), 5 + (88 << 4)]


def _conv(n, hw, ci, co, k=3, stride=1, dil=1, up=1, pad=1, subpix=0, ho=None):
    ho = ho if ho is not None else hw * up // stride
    return dict(N=n, H=hw, W=hw, Cin=ci, Ho=ho, Wo=ho, Cout=co, R=k, stride=stride, dil_in=dil, up=up, pad=pad, subpix=subpix)


# B = 16: the model's 3x3 layers, the image layers (3 -> 8 padded channels), the sub-pixel Upsample forward, the patch data gradients of the
# discriminator heads (k = s = 4, 32 and 64 channels of dy at 64^2 -> 256^2), a 1x1 conv, a stride-2 3x3, the nearest-2x gather
SHAPES = [_conv(16, 256, 128, 128), _conv(16, 256, 256, 128), _conv(16, 256, 128, 256), _conv(16, 128, 256, 256), _conv(16, 64, 512, 512),
          _conv(16, 32, 512, 512), _conv(16, 16, 512, 512), _conv(16, 256, 64, 64), _conv(16, 256, 128, 8), _conv(16, 256, 64, 8),
          _conv(16, 256, 8, 128), _conv(16, 128, 256, 1024, k=2, subpix=2), _conv(16, 64, 64, 32, k=4, dil=4, pad=3, ho=256),
          _conv(16, 64, 32, 64, k=4, dil=4, pad=3, ho=256), _conv(16, 64, 256, 256, k=1, pad=0), _conv(16, 128, 128, 128, stride=2, pad=0),
          _conv(16, 64, 256, 256, up=2), _conv(16, 128, 128, 128)]
# what only small or odd shapes reach: 64-row tiles, Cin not a multiple of 64 (conv_igemm_kernel), short-M tiles, true != padded channels
EXTRA = [_conv(16, 16, 128, 64), _conv(2, 16, 64, 96), _conv(16, 32, 32, 128), _conv(16, 32, 32, 64), _conv(16, 32, 32, 8),
         _conv(16, 16, 64, 128, k=1, pad=0), _conv(1, 16, 128, 128)]


def _cases():
    for dtype in (BF16, F16):
        for s in SHAPES + EXTRA:
            for hint in HINTS:
                for flags in ((0, 1, 2, 3, 4, 6) if hint == 0 else (0, 2)):     # bits: 1 residual, 2 GroupNorm partials, 4 gn_bwd
                    yield dict(s, dtype=dtype, split=1), hint, flags
    for s in SHAPES + EXTRA:                                                        # VQ_F16X2 (Cin in real channels), fp32 storage per split
        yield dict(s, dtype=F16X2, split=1), 0, 0
        yield dict(s, dtype=F16X2, split=1), 0, 2
    for split in (1, 3, 6):
        for s in (_conv(16, 64, 128, 128), _conv(16, 64, 64, 64), _conv(16, 64, 64, 8)):
            yield dict(s, dtype=F32, split=split), 0, 0


def _answers(lib, d, hint, flags):
    import vqgan_training_amd as vq
    desc = vq._lib.VqConvDesc()
    for k in ("N", "H", "W", "Cin", "Ho", "Wo", "Cout", "stride", "dil_in", "up", "subpix", "dtype", "split"):
        setattr(desc, k, d[k])
    desc.Cin_w, desc.Cout_w, desc.R, desc.S, desc.pad_t, desc.pad_l, desc.kernel_hint = d["Cin"], d["Cout"], d["R"], d["R"], d["pad"], d["pad"], hint
    probe = lib.dll.vq_debug_conv_plan
    probe.restype, probe.argtypes = C.c_int, [C.POINTER(vq._lib.VqConvDesc), C.c_int, C.POINTER(C.c_int), C.c_int]
    out = (C.c_int * len(PLAN))()
    assert probe(C.byref(desc), flags, out, len(PLAN)) == len(PLAN)
    return list(out), lib.dll.vq_conv_weight_layout(C.byref(desc)), lib.dll.vq_conv2d_gn_tile(C.byref(desc), GROUPS)


def _source_rows():
    """(family name, BC, BP, WC, WP, v0, v1, v2) of every release row of the plan -> instantiation tables, the fp32 rows once per split, and
    the families vq_conv2d_fwd launches outside the tables; plus the enum's name -> value map."""
    src = open(SOURCE).read()
    enum = re.search(r"enum ConvFamily \{(.*?)\};", src, re.S).group(1)
    names = [n.split("=")[0].strip() for n in re.sub(r"//[^\n]*", "", enum).split(",") if n.strip()]
    family = {n[len("CONV_"):]: i for i, n in enumerate(names)}
    rows = set()
    for macro in ("CONV_GENERIC_ROWS", "CONV_TILE_ROWS", "CONV_TILE_ROWS_NOT_X2"):
        body = re.search(r"#define %s\(X\)((?:[^\n]*\\\n)*[^\n]*)\n" % macro, src).group(1)
        found = re.findall(r"X\((\w+), (\d+), (\d+), (\d+), (\d+), (\w+), (\w+), (\w+)\)", body)
        assert found, macro
        for f, *t in found:
            for split, bk in ((1, 64), (3, 32), (6, 16)) if t[4] == "SPLIT" else ((None, None),):
                rows.add((f,) + tuple(int({"SPLIT": split, "BK": bk}.get(v, v)) for v in t))
    for f in sorted(set(re.findall(r"plan\.family == CONV_(\w+)\) return", src))):
        rows.add((f, 0, 0, 0, 0, 0, 0, 0))
    return rows, family


def test_conv_plan_table(emu_library):
    table = json.load(open(TABLE))
    assert table["desc"] == list(DESC) and table["plan"] == list(PLAN) and table["groups"] == GROUPS
    recorded = {tuple(r[:len(DESC) + 2]): r[len(DESC) + 2:] for r in table["rows"]}
    cases = list(_cases())
    assert len(recorded) == len(table["rows"]) == len(cases)
    for d, hint, flags in cases:
        want = recorded[tuple(d[k] for k in DESC) + (hint, flags)]
        plan, layout, gn_tile = _answers(emu_library, d, hint, flags)
        where = (d, hint, flags)
        assert plan == want[:len(PLAN)], where                                  # 1. the recorded plan
        assert [layout, gn_tile] == want[len(PLAN):], where
        p = dict(zip(PLAN, plan))
        assert layout == p["layout"], where                                     # 2. the queries read the plan ...
        if flags == 2:                                                          # ... vq_conv2d_gn_tile the one WITH partials requested,
            patch = d["dil_in"] > 1 and d["dil_in"] == d["R"]                   #     and answers 0 for a patch data gradient before it
            ok = d["Cout"] % GROUPS == 0 and d["Cout"] // GROUPS in (4, 8, 16, 32) and not patch
            assert gn_tile == (p["gn_row"] if ok else 0), where
            if p["gn_row"]:
                assert p["gn_row"] * p["gn_nw"] == p["gn_bp"] and (d["Ho"] * d["Wo"]) % p["gn_bp"] == 0, where


def test_every_release_instantiation_has_a_row():
    """3. A new row of the plan -> instantiation tables (or a new family) fails here until the table holds a descriptor that reaches it."""
    rows, family = _source_rows()
    assert len(rows) == 3 * 3 + 14 + 1 + 3, sorted(rows)       # fp32 tiles x splits, LDS-DMA tiles, the 128 x 256 tile, c8 / c8_x2 / patch dgrad
    table = json.load(open(TABLE))
    seen = {tuple(r[len(DESC) + 2:len(DESC) + 10]) for r in table["rows"]}
    missing = [r for r in sorted(rows) if (family[r[0]],) + r[1:] not in seen]
    assert not missing, missing


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    sys.path.insert(0, ROOT)
    import vqgan_training_amd as vq
    lib = vq._lib.VqLibrary(os.path.join(ROOT, "tests", "emu", "libvqhip_emu.so"))
    rows = []
    for d, hint, flags in _cases():
        plan, layout, gn_tile = _answers(lib, d, hint, flags)
        rows.append([d[k] for k in DESC] + [hint, flags] + plan + [layout, gn_tile])
    with open(TABLE, "w") as f:
        f.write('{"desc": %s, "plan": %s, "groups": %d,\n "rows": [\n' % (json.dumps(list(DESC)), json.dumps(list(PLAN)), GROUPS))
        f.write(",\n".join("  " + json.dumps(r) for r in rows) + "\n]}\n")
    print(len(rows), "rows")
