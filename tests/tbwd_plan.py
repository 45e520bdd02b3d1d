"""The backward launches of the temporal stack as data: the layer table of adx_unet_backward (csrc/unet.hip: build,
csrc/unet_train.hip: adx_unet_backward), the weight gradient's launch geometry (include/adx.h: adx_tconv_wgrad_plan_describe), the
data gradient's (adx_tconv_plan_describe on the descriptor dgrad_desc builds), and the op-level cases tests/test_gpu_tbwd.py runs.
tests/test_tbwd_plan_cpu.py checks -- without a GPU -- that the case list takes both sides of every geometry flip."""
import ctypes as C
from collections import namedtuple

WG_FIELDS = ("per4", "nfo", "n_ci_tiles", "n_co_tiles", "tiles", "nsplit", "nb", "sbt", "pl", "lp", "rs", "lds_stage", "lds_red",
             "lds_bytes", "grid", "_15")
DESC_FIELDS = ("kind", "taps", "stride", "pad", "c0", "c1", "cout", "lin", "lout", "groups", "eps", "w_layout", "w_flip", "exact",
               "lin_valid", "lout_valid")
Desc = namedtuple("Desc", DESC_FIELDS)

# the configurations whose every layer tests/test_tbwd_plan_cpu.py sweeps over batches 1..B_MAX: (H, dim, mults)
SWEEP_CONFIGS = ((16, 64, (1, 2, 4, 8)), (32, 64, (1, 2, 4, 8)), (24, 64, (1, 2, 4, 8)), (40, 64, (1, 2, 4, 8)),
                 (56, 64, (1, 2, 4, 8)), (64, 64, (1, 2, 4, 8)), (32, 32, (1, 2, 4, 8)), (32, 128, (1, 2, 4, 8)))
B_MAX = 160


def pow2_ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def conv_desc(kind, taps, stride, pad, c0, c1, cout, lin, lout, groups=0):
    """csrc/unet.hip: conv_desc -- lin / lout are the REAL lengths; lengths that are not powers of two run on the next one with
    the real ones as masks."""
    pi, po = pow2_ceil(lin), pow2_ceil(lout)
    masked = pi != lin or po != lout
    return Desc(kind, taps, stride, pad, c0, c1, cout, pi, po, groups, 1e-5, 0, 0, 0, lin if masked else 0, lout if masked else 0)


def mirror_desc(d):
    """The ConvTranspose1d weight gradient's descriptor (csrc/unet_train.hip: `m`): the mirrored strided conv, x and dy swapped."""
    assert d.kind == 1
    return Desc(0, d.taps, d.stride, d.pad, d.cout, 0, d.c0 + d.c1, d.lout, d.lin, 0, d.eps, 0, 0, 0, d.lout_valid, d.lin_valid)


def dgrad_desc(d):
    """csrc/unet_train.hip: dgrad_desc -- the data gradient of a conv launch as a conv of the same family, exact-fp32."""
    base = dict(c0=d.cout, c1=0, cout=d.c0 + d.c1, lin=d.lout, lout=d.lin, taps=d.taps, groups=0, eps=d.eps, exact=1,
                lin_valid=d.lout_valid, lout_valid=d.lin_valid)
    if d.kind == 0 and d.stride == 1:
        return Desc(kind=0, stride=1, pad=d.taps - 1 - d.pad, w_layout=1, w_flip=1, **base)
    if d.kind == 0:
        return Desc(kind=1, stride=d.stride, pad=d.pad, w_layout=0, w_flip=0, **base)
    return Desc(kind=0, stride=d.stride, pad=d.pad, w_layout=0, w_flip=0, **base)


def tlin_dgrad_desc(sum_c, two_dim):
    """csrc/unet_train.hip: g_tlin."""
    return Desc(0, 1, 1, 0, sum_c, 0, two_dim, 1, 1, 0, 1e-5, 1, 0, 1, 0, 0)


def c_desc(d):
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    return L.TConvDesc(*d)


# one backward launch group of adx_unet_backward: `d` the forward conv, `wgrad` the descriptor tconv_wgrad runs (mirrored for the
# upsamples), `dgrad` the data gradient's (None: the input needs no gradient), `x` how the weight gradient reads its input
# ("dense", "bhd": the trajectory in place as [B][H][D], "tlin": one position, position stride 0)
Layer = namedtuple("Layer", "name d wgrad dgrad x")


def layer_table(H, dim=64, mults=(1, 2, 4, 8), transition_dim=7, guidance=0):
    """Every conv launch adx_unet_backward differentiates, in the order csrc/unet.hip: build creates the layers."""
    n = len(mults)
    assert H % (1 << (n - 1)) == 0
    dims = [transition_dim] + [dim * m for m in mults]
    out, sum_c = [], 0

    def add(name, d, need_dx=True, x="dense"):
        out.append(Layer(name, d, mirror_desc(d) if d.kind == 1 else d, dgrad_desc(d) if need_dx else None, x))

    def block(name, c0, c1, cout, ln, need_dx=True, x="dense"):
        nonlocal sum_c
        add(name + ".a", conv_desc(0, 5, 1, 2, c0, c1, cout, ln, ln, 8), need_dx, x)
        add(name + ".b", conv_desc(0, 5, 1, 2, cout, 0, cout, ln, ln, 8))
        if c0 + c1 != cout:
            add(name + ".r", conv_desc(0, 1, 1, 0, c0, c1, cout, ln, ln), need_dx, x)
        sum_c += cout

    ln = H
    for i in range(n):
        ci, co = dims[i], dims[i + 1]
        block(f"down{i}.0", ci, 0, co, ln, need_dx=i > 0, x="dense" if i > 0 else "bhd")   # the noisy trajectory needs no gradient
        block(f"down{i}.1", co, 0, co, ln)
        if i < n - 1:
            add(f"down{i}.down", conv_desc(0, 3, 2, 1, co, 0, co, ln, ln // 2))
            ln //= 2
    for k in range(2):
        block(f"mid.{k}", dims[n], 0, dims[n], ln)
    ul = ln
    for i in range(n - 1):
        ci, co = dims[n - 1 - i], dims[n - i]
        block(f"up{i}.0", co, co, ci, ul)
        block(f"up{i}.1", ci, 0, ci, ul)
        add(f"up{i}.up", conv_desc(1, 4, 2, 1, ci, 0, ci, ul, ul * 2))
        ul *= 2
    fin = dims[1] if n > 1 else dims[n]
    add("head0", conv_desc(0, 5, 1, 2, fin, 0, fin, ul, ul, 8))
    add("head1", conv_desc(0, 1, 1, 0, fin, 0, 3 if guidance == 2 else transition_dim, ul, ul))
    tl = conv_desc(0, 1, 1, 0, 2 * dim, 0, sum_c, 1, 1)
    out.append(Layer("tlin", tl, tl, tlin_dgrad_desc(sum_c, 2 * dim), "tlin"))
    return out


def distinct_launches(table):
    """(wgrad descriptors, dgrad descriptors) of a layer table without repeats."""
    return sorted({l.wgrad for l in table}), sorted({l.dgrad for l in table if l.dgrad is not None})


def wgrad_plan(d, batch):
    """adx_tconv_wgrad_plan_describe as a dict."""
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    ints = (L.i32 * len(WG_FIELDS))()
    cd = c_desc(d)
    L.check(L.lib().adx_tconv_wgrad_plan_describe(C.byref(cd), batch, ints), "adx_tconv_wgrad_plan_describe")
    return dict(zip(WG_FIELDS, ints))


def wgrad_flips(d, batch, p=None):
    """What of a weight-gradient launch a kernel bug could hide behind: the flips the case list must take both sides of."""
    p = p or wgrad_plan(d, batch)
    last = batch - (p["nsplit"] - 1) * p["nb"]                   # samples of the last split
    # a split with several super-tiles whose last one is ragged (nsamp < sbt)
    ragged = any(n > p["sbt"] and n % p["sbt"] != 0 for n in ({p["nb"], last} if p["nsplit"] > 1 else {last}))
    several = any(n > p["sbt"] for n in ({p["nb"], last} if p["nsplit"] > 1 else {last}))
    return {("nsplit>1", p["nsplit"] > 1), ("supertiles", "ragged" if ragged else ("several" if several else "one")),
            ("per4", p["per4"]), ("short_last_split", p["nsplit"] > 1 and last < p["nb"]), ("nfo", p["nfo"]),
            ("cin%16", (d.c0 + d.c1) % 16 != 0), ("cout<16", d.cout < 16)}


# what the case list must reach of the weight gradient
WGRAD_REQUIRED = ({("nsplit>1", v) for v in (False, True)} | {("supertiles", v) for v in ("one", "ragged")} |
                  {("per4", v) for v in (1, 2, 4)} | {("short_last_split", v) for v in (False, True)} |
                  {("nfo", v) for v in (1, 2, 4)} | {("cin%16", v) for v in (False, True)} | {("cout<16", v) for v in (False, True)})


def dgrad_plan(g, batch):
    """The one launch record of the data gradient (tests/unet_plan.py: FIELDS) plus what follows from it: nf, nw."""
    import unet_plan as UP
    recs = UP.tconv_plan(c_desc(g), batch)
    assert len(recs) == 1 and recs[0]["family"] == "exact", recs          # exact = 1: one launch of the exact-fp32 kernel
    r = dict(recs[0])
    cout_pad = (g.cout + 15) // 16 * 16
    r["nf"] = cout_pad // 16 // r["ctiles"]
    nkb = g.taps * r["cin_pad"] // 16
    r["nw"] = 16 if nkb >= 64 else (8 if nkb >= 32 else 4)          # csrc/tconv.hip: tconv_tile, waves that split K
    return r


def dgrad_flips(g, batch, r=None):
    r = r or dgrad_plan(g, batch)
    return {("rows%bt", r["rows_mod_bt"] != 0), ("nf", r["nf"]), ("chunks>=2", r["chunks"] >= 2), ("nw", r["nw"])}


def dgrad_form(g):
    """Which of dgrad_desc's forms a descriptor is."""
    if g.lin == 1 and g.lout == 1:
        return "tlin"
    if g.kind == 1:
        return "of_strided"                # kind 1: a strided conv's gradient
    return "of_upsample" if g.stride == 2 else "of_stride1"


# ------------------------------------------------------------------------------------------------------------------------
# The op-level cases of tests/test_gpu_tbwd.py.  Every case is one launch (run twice for the weight gradient).
# wgrad: (name, forward descriptor `d` -- mirrored inside for kind 1 --, batch, how x is read)
_W = conv_desc
WGRAD_CASES = (
    ("w512.L4.b37", _W(0, 5, 1, 2, 512, 0, 512, 4, 4, 8), 37, "dense"),        # nsplit = 1, two super-tiles, tail of 5
    ("w512.L2.b67", _W(0, 5, 1, 2, 512, 0, 512, 2, 2, 8), 67, "dense"),        # per4 = 2, two super-tiles, tail of 3
    ("w256-512.L4.b70", _W(0, 5, 1, 2, 256, 0, 512, 4, 4, 8), 70, "dense"),    # nsplit = 2, nb = 35, tail of 3
    ("wcat.L8.b35", _W(0, 5, 1, 2, 256, 256, 128, 8, 8, 8), 35, "dense"),      # concat, last split of 8 against nb = 9
    ("w7-64.L32.b64", _W(0, 5, 1, 2, 7, 0, 64, 32, 32, 8), 64, "bhd"),         # x in place as [B][H][D], cin % 16 != 0
    ("w64-7.L32.b9", _W(0, 1, 1, 0, 64, 0, 7, 32, 32), 9, "dense"),            # taps 1, nfo = 1, cout < 16
    ("wdown256.L8.b45", _W(0, 3, 2, 1, 256, 0, 256, 8, 4), 45, "dense"),       # stride 2
    ("wup256.L4.b45", _W(1, 4, 2, 1, 256, 0, 256, 4, 8), 45, "dense"),         # the ConvTranspose weight: mirrored, taps 4
    ("wtlin.b5", _W(0, 1, 1, 0, 128, 0, 1984, 1, 1), 5, "tlin"),               # per4 = 4, position stride 0
    ("wtlin.b131", _W(0, 1, 1, 0, 128, 0, 1984, 1, 1), 131, "tlin"),
    ("w64-32.L16.b3", _W(0, 1, 1, 0, 64, 0, 32, 16, 16), 3, "dense"),          # nfo = 2
    # real lengths below the padded ones (H = 24: 24, 12, 6, 3; H = 40: 40, 20, 10, 5)
    ("w256.L6of8.b37", _W(0, 5, 1, 2, 256, 0, 256, 6, 6, 8), 37, "dense"),
    ("wdown256.L6of8.b45", _W(0, 3, 2, 1, 256, 0, 256, 6, 3), 45, "dense"),
    ("wup256.L3of4.b45", _W(1, 4, 2, 1, 256, 0, 256, 3, 6), 45, "dense"),
    ("w512.L5of8.b33", _W(0, 5, 1, 2, 512, 0, 512, 5, 5, 8), 33, "dense"),
    ("wup512.L5of8.b33", _W(1, 4, 2, 1, 512, 0, 512, 5, 10), 33, "dense"),
)

# dgrad: (name, forward descriptor `d` whose data gradient runs, batch, accumulate into a non-zero buffer (res == y))
DGRAD_CASES = (
    ("g512.L4.b37", _W(0, 5, 1, 2, 512, 0, 512, 4, 4, 8), 37, False),          # one chunk (single wave of workgroups), rows % bt != 0
    ("g512.L4.b67", _W(0, 5, 1, 2, 512, 0, 512, 4, 4, 8), 67, True),           # two chunks
    ("g512.L4.b44", _W(0, 5, 1, 2, 512, 0, 512, 4, 4, 8), 44, False),          # two chunks, rows % bt == 0
    ("gdown256.L16.b130", _W(0, 3, 2, 1, 256, 0, 256, 16, 8), 130, True),      # kind 1: a strided conv's gradient; nf = 4
    ("gup256.L8.b45", _W(1, 4, 2, 1, 256, 0, 256, 4, 8), 45, True),            # kind 0, stride 2: an upsample's gradient
    ("g128.L32.b128", _W(0, 5, 1, 2, 128, 0, 128, 32, 32, 8), 128, False),     # nf = 2
    ("g256.L16.b129", _W(0, 5, 1, 2, 256, 0, 256, 16, 16, 8), 129, True),      # nf = 4
    ("g64-7.L32.b9", _W(0, 1, 1, 0, 64, 0, 7, 32, 32), 9, False),              # head1: nw = 4
    ("gcat.L8.b35", _W(0, 5, 1, 2, 256, 256, 128, 8, 8, 8), 35, False),        # the concat's gradient (one tensor, split later)
    ("g256.L6of8.b37", _W(0, 5, 1, 2, 256, 0, 256, 6, 6, 8), 37, True),
    ("gdown256.L6of8.b45", _W(0, 3, 2, 1, 256, 0, 256, 6, 3), 45, False),
    ("gup512.L5of8.b33", _W(1, 4, 2, 1, 512, 0, 512, 5, 10), 33, True),
)
# the fused time Linear's gradient: (name, sum_c, 2 dim, batch)
TLIN_DGRAD_CASES = (("gtlin.b5", 1984, 128, 5), ("gtlin.b131", 1984, 128, 131))

# adx_gn_mish_backward_ex: (name, B, C, L, L_valid (0: L), with dtb, with dbias)
GN_CASES = (
    ("gn.cg8.L8.b37", 37, 64, 8, 0, True, True),             # cg * L = 64
    ("gn.cg8.L16.b37", 37, 64, 16, 0, False, True),          # 128
    ("gn.cg16.L16.b128", 128, 128, 16, 0, True, False),      # 256
    ("gn.cg64.L8.b37", 37, 512, 8, 0, True, True),           # 512
    ("gn.cg8.L64.b37", 37, 64, 64, 0, True, True),           # L = 64: one chunk holds every position of a channel, dtb stored
    ("gn.cg64.L5of8.b128", 128, 512, 8, 5, True, True),      # L_valid < L
    ("gn.cg8.L40of64.b37", 37, 64, 64, 40, True, True),
)
# adx_bias_grad_ex: (name, B, C, L, L_valid, layout): "dense" [B][C][L]; "tlin" [B][C], one position with stride 0
BIAS_CASES = (("b7.L32.b37", 37, 7, 32, 0, "dense"), ("b7.L24of32.b70", 70, 7, 32, 24, "dense"), ("btlin.b300", 300, 1984, 1, 0, "tlin"))


def n_cases():
    return len(WGRAD_CASES) + len(DGRAD_CASES) + len(TLIN_DGRAD_CASES) + len(GN_CASES) + len(BIAS_CASES)


def wgrad_case_flips(cases=WGRAD_CASES):
    out = set()
    for _, d, batch, _x in cases:
        out |= wgrad_flips(mirror_desc(d) if d.kind == 1 else d, batch)
    return out


def dgrad_case_flips(cases=DGRAD_CASES, tlin=TLIN_DGRAD_CASES):
    out = set()
    for _, d, batch, _acc in cases:
        out |= dgrad_flips(dgrad_desc(d), batch)
    for _, sum_c, two_dim, batch in tlin:
        out |= dgrad_flips(tlin_dgrad_desc(sum_c, two_dim), batch)
    return out


def dgrad_required(configs=SWEEP_CONFIGS, b_max=B_MAX):
    """Both sides of rows % bt and of chunks, and every nf and nw the data gradients of the swept configurations reach."""
    need = {("rows%bt", False), ("rows%bt", True), ("chunks>=2", False), ("chunks>=2", True)}
    for H, dim, mults in configs:
        for g in distinct_launches(layer_table(H, dim, mults))[1]:
            for batch in range(1, b_max + 1):
                r = dgrad_plan(g, batch)
                need |= {("nf", r["nf"]), ("nw", r["nw"])}
    return need
