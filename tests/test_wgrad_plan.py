"""wgrad_plan (csrc/conv_wgrad.hip): the one function that says which kernel computes the weight gradient of a conv descriptor, over which
split-K grid, which reduction sums the slabs and how the workspace is laid out.  tests/golden/wgrad_plan_table.json records its answers
— and vq_conv2d_wgrad_workspace's, which Python allocates by — for the model's layers and the shapes that reach every instantiation and
every reduction, under every hint the kernel tests use.  The plan is read through vq_debug_wgrad_plan, which only `make ABLATE=1` /
emulator builds carry: CPU only.

Re-record after a deliberate change of the selection:  python tests/test_wgrad_plan.py --record
"""
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "wgrad_plan_table.json")
CSRC = os.path.join(ROOT, "vqgan-training_amd", "csrc")
BF16, F32, F16, F16X2 = 0, 1, 2, 3
DESC = ("N", "H", "W", "Cin", "Ho", "Wo", "Cout", "Cin_w", "Cout_w", "R", "stride", "dil_in", "up", "pad", "dtype", "split")
PLAN = ("family", "dtype", "BT", "NW", "GEN", "SEG", "STAG", "X3", "SPLIT", "NBUF", "n_ct", "n_cit", "nsplit", "pix_per_split", "xcd_tiles",
        "grid_x", "grid_y", "lds_bytes", "fused_bias", "reduce", "lpi", "red_blocks", "bias_blocks", "slab_real", "off_bias", "off_colsum", "total")
FAMILY = {"NONE": 0, "C8_X2": 1, "C8": 2, "TAP3": 3, "GLDS": 4, "GENERIC": 5}             # enum WgradFamily
REDUCE = {"OWN": 0, "SCALAR": 1, "VEC4": 2, "VEC9": 3, "X2": 4}                            # enum WgradReduce
DTYPE = {"VQ_BF16": BF16, "VQ_F32": F32, "VQ_F16": F16}
# kernel_hint (include/vqhip.h): slow reduction, no three-tap kernel, virtual VQ_F16X2 form, unstaggered staging, forced one-tap tiles,
# forced split counts (bits 16..: one that leaves lanes-per-item at 2, an odd one, one that is no multiple of 8 until clamped), an unknown bit
HINTS = [0, 1, 4, 8, 16, 64, 128, 256, 2 << 16, 3 << 16, 24 << 16, 2]


def _conv(n, hw, ci, co, k=3, stride=1, up=1, pad=1, ho=None, ci_w=None, co_w=None):
    ho = ho if ho is not None else hw * up // stride
    return dict(N=n, H=hw, W=hw, Cin=ci, Ho=ho, Wo=ho, Cout=co, Cin_w=ci_w or ci, Cout_w=co_w or co, R=k, stride=stride, dil_in=1, up=up, pad=pad)


# B = 16: the model's 3x3 layers at 128 / 256 / 512 channels from 256^2 down to 16^2, the nearest-2x layer, the transposed form of the Upsample
# conv (4x4 / stride 2, roles swapped: 16 taps reach the 256 tile from 16384 pixels), a 1x1, a stride-2 3x3
MODEL = [_conv(16, 256, 128, 128), _conv(16, 128, 128, 256), _conv(16, 128, 256, 256), _conv(16, 64, 256, 512), _conv(16, 64, 512, 512),
         _conv(16, 32, 512, 512), _conv(16, 16, 512, 512), _conv(16, 64, 256, 256, up=2), _conv(16, 64, 512, 512, k=4, stride=2, ho=32),
         _conv(16, 256, 256, 256, k=4, stride=2, ho=128), _conv(16, 64, 256, 256, k=1, pad=0), _conv(16, 128, 128, 128, stride=2, pad=0)]
# three-tap forms: rows of 16 / 32 / 64 pixels (SEG 4 / 5 / 6), rows of 8 pixels and a 12 x 12 image (GEN)
TAP3 = [_conv(16, 16, 128, 128), _conv(16, 32, 128, 128), _conv(16, 64, 128, 128), _conv(16, 8, 128, 128), _conv(16, 12, 128, 128)]
# one-tap tiles: 64 (C = 64 and 192), 128, 256 on its 131072-pixel threshold (MODEL's 1x1 is below it); 64 channels under nine taps
GLDS = [_conv(16, 64, 64, 64, k=1, pad=0), _conv(16, 64, 192, 192, k=1, pad=0), _conv(16, 64, 128, 128, k=1, pad=0),
        _conv(8, 128, 256, 256, k=1, pad=0), _conv(16, 256, 64, 64)]
# the generic kernel: C = 32 and 96, rows of 10 pixels at 128 channels (neither LDS-DMA kernel), a pair >= 128 that is no multiple of 64
GENERIC = [_conv(16, 32, 32, 32), _conv(2, 16, 96, 96), _conv(32, 10, 128, 128), _conv(16, 32, 136, 136)]
# both orientations of the 8-channel kernels (Cin_w / Cout_w = 3), 64 and 128 wide channels; the same Cin_w on rows the c8 kernel refuses
C8 = [_conv(16, 256, 8, 64, ci_w=3), _conv(16, 256, 8, 128, ci_w=3), _conv(16, 256, 64, 8, co_w=3), _conv(16, 256, 128, 8, co_w=3),
      _conv(16, 16, 8, 64, ci_w=3)]
# reductions: 512 x 384 stays below wgrad_reduce9_kernel's 512 x 512; short reductions (fewer than 8 splits possible; one split)
REDUCE_SHAPES = [_conv(16, 16, 384, 512), _conv(1, 32, 128, 128), _conv(1, 16, 64, 64), _conv(1, 16, 256, 256), _conv(4, 16, 128, 128)]
# VQ_F16X2 (real channel counts): three-tap native form at 64 and 128 channels, one-tap native form at 128 and 256 virtual channels,
# the 64-wide tile that keeps the virtual form, 256 channels (one lane per item under hint +8), a 12 x 12 image (GEN), the 8-channel twins
X2 = [_conv(16, 64, 64, 64), _conv(16, 32, 128, 128), _conv(16, 64, 64, 64, k=1, pad=0), _conv(8, 128, 128, 128, k=1, pad=0),
      _conv(16, 64, 32, 32, k=1, pad=0), _conv(16, 32, 256, 256), _conv(1, 16, 64, 64), _conv(16, 12, 64, 64), _conv(16, 256, 8, 32, ci_w=3),
      _conv(16, 256, 8, 64, ci_w=3), _conv(16, 256, 8, 128, ci_w=3), _conv(16, 256, 64, 8, co_w=3)]
SHAPES16 = MODEL + TAP3 + GLDS + GENERIC + C8 + REDUCE_SHAPES


def _flags(hint):                        # bits: 1 a bias gradient is wanted, 2 dw is 16-byte aligned
    return (0, 1, 2, 3) if hint == 0 else (0, 3)


def _cases():
    for s in SHAPES16:                                                              # the selection does not read bf16 / binary16 apart
        for hint in (0, 16) if s in TAP3 else (0,):                                 # (but the unstaggered three-tap rows exist per type)
            for flags in _flags(hint):
                yield dict(s, dtype=BF16, split=1), hint, flags
        for hint in HINTS:
            for flags in _flags(hint):
                yield dict(s, dtype=F16, split=1), hint, flags
    for s in X2:
        for hint in HINTS:
            for flags in _flags(hint):
                yield dict(s, dtype=F16X2, split=1), hint, flags
    for split in (1, 3, 6, 2):                                                      # fp32 storage per split; 2 is none (WG_NONE)
        for s in (_conv(16, 64, 128, 128), _conv(16, 64, 64, 64), _conv(16, 256, 8, 64, ci_w=3)):
            for flags in _flags(0):
                yield dict(s, dtype=F32, split=split), 0, flags


def _answers(lib, d, hint, flags):
    import vqgan_training_amd as vq
    desc = vq._lib.VqConvDesc()
    for k in ("N", "H", "W", "Cin", "Ho", "Wo", "Cout", "Cin_w", "Cout_w", "stride", "dil_in", "up", "dtype", "split"):
        setattr(desc, k, d[k])
    desc.R, desc.S, desc.pad_t, desc.pad_l, desc.kernel_hint = d["R"], d["R"], d["pad"], d["pad"], hint
    probe = lib.dll.vq_debug_wgrad_plan
    probe.restype, probe.argtypes = C.c_int, [C.POINTER(vq._lib.VqConvDesc), C.c_int, C.POINTER(C.c_longlong), C.c_int]
    query = lib.dll.vq_conv2d_wgrad_workspace
    query.restype, query.argtypes = C.c_size_t, [C.POINTER(vq._lib.VqConvDesc)]
    out = (C.c_longlong * len(PLAN))()
    assert probe(C.byref(desc), flags, out, len(PLAN)) == len(PLAN)
    return list(out), query(C.byref(desc))


def _macro(src, name):
    """Body of a (possibly continued) #define, comments removed."""
    body = re.search(r"#define %s\([^)]*\)((?:[^\n]*\\\n)*[^\n]*)\n" % name, src).group(1)
    return re.sub(r"/\*.*?\*/", "", body)


def _source_rows():
    """Every row of the plan -> instantiation tables as (family, dtype, BT, NW, GEN, SEG, STAG, X3, SPLIT, NBUF), the 8-channel kernels' as
    (dtype, BT), the reductions' as (kind, lpi), and the number of 8-channel reductions."""
    src = open(os.path.join(CSRC, "conv_wgrad.hip")).read()
    forms = _macro(src, "WGRAD_TAP3_FORMS")
    rows = set()
    for macro, dtypes in (("WGRAD_ROWS_16", (BF16, F16)), ("WGRAD_ROWS_F16_X3", (F16,)), ("WGRAD_ROWS_F32", (F32,))):
        body = re.sub(r"WGRAD_TAP3_FORMS\(X, (\d+), (\d+), (\d+)\)",
                      lambda m: forms.replace("NW", m.group(1)).replace("STAG", m.group(2)).replace("X3", m.group(3)), _macro(src, macro))
        found = re.findall(r"X\((\w+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)", body)
        assert found and len(found) == body.count("X("), macro
        rows |= {(FAMILY[f], dt) + tuple(int(v) for v in t) for f, *t in found for dt in dtypes}
    reductions = {(REDUCE[k], int(lpi)) for k, lpi in re.findall(r"X\((\w+), (\d), wgrad_reduce", _macro(src, "WGRAD_REDUCE_ROWS"))}
    small = open(os.path.join(CSRC, "conv_small.hip")).read()
    c8 = {(DTYPE[dt], int(bt)) for dt, bt in re.findall(r"X\((\w+), (\d+)\)", _macro(small, "WGRAD_C8_ROWS"))}
    # nothing is launched past the tables: each kernel template is named once (its WG_INST_ row form / the 8-channel launcher), each reduction by its row
    host = re.sub(r"//[^\n]*", "", src[src.index("host side: plan, launch, queries"):])
    for text, kernel in ((host, "conv_wgrad_kernel<"), (host, "conv_wgrad_glds_kernel<"), (host, "conv_wgrad3_kernel<"), (small, "((wgrad_c8_kernel<")):
        assert text.count(kernel) == 1, kernel
    assert "hipLaunchKernelGGL(wgrad_reduce" not in host and host.count("hipLaunchKernelGGL(KERNEL,") == 2
    return rows, c8, reductions, len(re.findall(r"hipLaunchKernelGGL\(wgrad_c8_reduce\w*kernel", small))


def test_wgrad_plan_table(emu_library):
    assert "VQ_WGRAD_CUS" not in os.environ, "the recorded plans are those of 256 CUs"
    table = json.load(open(TABLE))
    assert table["desc"] == list(DESC) and table["plan"] == list(PLAN)
    recorded = {tuple(r[:len(DESC) + 2]): r[len(DESC) + 2:] for r in table["rows"]}
    cases = list(_cases())
    assert len(recorded) == len(table["rows"]) == len(cases)
    for d, hint, flags in cases:
        want = recorded[tuple(d[k] for k in DESC) + (hint, flags)]
        plan, need = _answers(emu_library, d, hint, flags)
        where = (d, hint, flags)
        assert plan == want[:len(PLAN)], where                                  # 1. the recorded plan
        assert [need] == want[len(PLAN):], where
        p = dict(zip(PLAN, plan))
        assert need == p["total"], where                                        # 2. the query returns the plan's total (whatever the call flags)
        split_k = p["family"] not in (FAMILY["C8"], FAMILY["C8_X2"])
        assert 0 < p["off_bias"] <= p["off_colsum"] < p["total"] and (p["off_bias"] < p["off_colsum"]) == split_k, where
        assert p["off_bias"] % 256 == 0 and p["off_colsum"] % 256 == 0, where
        if split_k:                                                             # 3. the split covers the pixels in whole 64-pixel chunks
            M = d["N"] * d["Ho"] * d["Wo"]
            assert p["nsplit"] * p["pix_per_split"] >= M > (p["nsplit"] - 1) * p["pix_per_split"] and p["pix_per_split"] % 64 == 0, where
            lds_dma = p["family"] in (FAMILY["TAP3"], FAMILY["GLDS"])
            tiles = p["n_ct"] * p["n_cit"] * (3 if p["family"] == FAMILY["TAP3"] else d["R"] * d["R"])
            if lds_dma and p["xcd_tiles"] == 0:                                 # an XCD owns splits: whole groups of 8 splits
                assert p["grid_x"] % (8 * tiles) == 0 and p["grid_x"] >= p["nsplit"] * tiles, where
            if not lds_dma:
                assert (p["xcd_tiles"], p["grid_x"], p["grid_y"], p["fused_bias"]) == (0, tiles, p["nsplit"], 0), where
            assert p["fused_bias"] in (0, flags & 1) and (p["bias_blocks"] > 0) == (p["fused_bias"] == 1), where


def test_every_release_instantiation_has_a_row():
    """4. A new row of the plan -> instantiation tables (or a launch past them) fails here until the table holds a descriptor that reaches it."""
    rows, c8, reductions, c8_reductions = _source_rows()
    assert len([r for r in rows if r[0] == FAMILY["GENERIC"]]) == 10 and len([r for r in rows if r[0] == FAMILY["GLDS"]]) == 8
    assert len([r for r in rows if r[0] == FAMILY["TAP3"]]) == 20 and len(rows) == 38
    assert len(c8) == 4 and len(reductions) == 10 and c8_reductions == 2
    table = json.load(open(TABLE))
    plans = [dict(zip(PLAN, r[len(DESC) + 2:])) for r in table["rows"]]
    seen = {tuple(p[k] for k in PLAN[:10]) for p in plans}
    assert not [r for r in sorted(rows) if r not in seen]
    assert not [r for r in sorted(c8) if not any(p["family"] == FAMILY["C8"] and (p["dtype"], p["BT"]) == r for p in plans)]
    assert {p["BT"] for p in plans if p["family"] == FAMILY["C8_X2"]} == {64, 128}
    assert not [r for r in sorted(reductions) if not any((p["reduce"], p["lpi"]) == r for p in plans)]
    assert {p["xcd_tiles"] for p in plans} == {0, 1, 2}


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    sys.path.insert(0, ROOT)
    import vqgan_training_amd as vq
    lib = vq._lib.VqLibrary(os.path.join(ROOT, "tests", "emu", "libvqhip_emu.so"))
    rows = []
    for d, hint, flags in _cases():
        plan, need = _answers(lib, d, hint, flags)
        rows.append([d[k] for k in DESC] + [hint, flags] + plan + [need])
    with open(TABLE, "w") as f:
        f.write('{"desc": %s, "plan": %s,\n "rows": [\n' % (json.dumps(list(DESC)), json.dumps(list(PLAN))))
        f.write(",\n".join("  " + json.dumps(r) for r in rows) + "\n]}\n")
    print(len(rows), "rows")
