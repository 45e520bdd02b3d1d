"""The launch plan of an eval UNet forward (include/adx.h: adx_unet_plan_describe) as Python records, and the rule that turns
the plans of rows 1..R_MAX into the row counts the GPU tests run (tests/test_unet_plan_cpu.py, tests/test_gpu_unet_rows.py).
The export needs no GPU: it is the forward's own host code with a recorder in place of the launches."""
import ctypes as C

R_MAX = 640          # above the largest threshold the export shows (512 rows: the K-split kernel's one-workgroup-per-CU budget at
                     # two positions, horizon 16; tests/test_unet_plan_cpu.py checks that nothing new appears up to 2048 rows)

FIELDS = ("group", "block", "conv", "family", "bt", "row_tiles", "rows_mod_bt", "ctiles", "grid", "ksplit", "reduce", "chunks",
          "vec_stage", "fast_epi", "ntap", "block_b", "conv_b", "ctiles_b", "ck", "cin_pad", "part_floats", "part_off", "lds_bytes",
          "lout", "cout", "aux", "_26", "_27")
FAMILIES = ("aux", "pipeline", "chain", "ksplit", "shortk", "shortk_pair", "mixed", "generic", "exact", "reduce")
CONVS = {-1: "-", 0: "a", 1: "b", 2: "r", 3: "down", 4: "up", 5: "head0", 6: "head1", 7: "tlin", 8: "qkv", 9: "attn_out", 10: "level",
         11: "run"}
ASSUME_PACKED, TIME_BIAS = 1, 2
# what of a record is a decision (the rest follows from the row count: row_tiles, rows_mod_bt, grid, the footprints)
SIGNATURE = ("family", "bt", "ctiles", "ksplit", "reduce", "chunks", "vec_stage", "fast_epi", "ntap", "block_b", "conv_b", "ctiles_b",
             "ck", "aux")
# families whose launch gives every row tile `bt` samples, real or not (the pipeline holds the whole batch in one tile)
TILED = ("chain", "ksplit", "shortk", "shortk_pair", "mixed", "exact")

# the configurations tests/test_gpu_unet_rows.py runs: (H, dim, mults, guidance).  H = 16 and 32 at the default width under both
# guidance modes, every other configuration under one (the plan does not depend on the mode; tests/test_unet_plan_cpu.py)
GPU_CONFIGS = (
    (16, 64, (1, 2, 4, 8), "NO_GUIDANCE"), (16, 64, (1, 2, 4, 8), "FREE_GUIDANCE"),
    (32, 64, (1, 2, 4, 8), "NO_GUIDANCE"), (32, 64, (1, 2, 4, 8), "FREE_GUIDANCE"),
    (24, 64, (1, 2, 4, 8), "FREE_GUIDANCE"), (64, 64, (1, 2, 4, 8), "NO_GUIDANCE"),
    (16, 64, (1, 2, 4), "FREE_GUIDANCE"), (24, 64, (1, 2, 4), "NO_GUIDANCE"),
    (32, 64, (1, 2, 4), "NO_GUIDANCE"), (64, 64, (1, 2, 4), "FREE_GUIDANCE"),
)

GUIDANCE = {"NO_GUIDANCE": 0, "FREE_GUIDANCE": 1, "CLASSIFIER_GUIDANCE": 2}


def _records(ints, n):
    out = []
    for i in range(n):
        r = dict(zip(FIELDS, ints[i * len(FIELDS):(i + 1) * len(FIELDS)]))
        r["family"] = FAMILIES[r["family"]]
        out.append(r)
    return out


def make_handle(horizon, dim=64, mults=(1, 2, 4, 8), use_cond="NO_GUIDANCE", transition_dim=7):
    """A native UNet object for the plan alone (no weights, no device)."""
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    cfg = L.UnetConfig()
    cfg.horizon, cfg.transition_dim, cfg.dim, cfg.n_mults, cfg.guidance = horizon, transition_dim, dim, len(mults), GUIDANCE[use_cond]
    for i, m in enumerate(mults):
        cfg.dim_mults[i] = m
    h = L.vp()
    L.check(L.lib().adx_unet_create(C.byref(cfg), C.byref(h)), "adx_unet_create")
    return h


def plan(handle, rows, flags=ASSUME_PACKED):
    """One dict per launch of an eval forward of `rows` rows, in launch order."""
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    cap = 256
    ints, n = (L.i32 * (cap * len(FIELDS)))(), L.i32(0)
    L.check(L.lib().adx_unet_plan_describe(handle, rows, flags, C.byref(n), ints, cap), "adx_unet_plan_describe")
    return _records(ints, n.value)


def tconv_plan(desc, batch, scratch_floats=0, tickets=False):
    """The same for one ops.tconv call (adx_tconv_plan_describe)."""
    from autonomous_driving_with_diffusion_model_amd import _lib as L
    ints, n = (L.i32 * (4 * len(FIELDS)))(), L.i32(0)
    L.check(L.lib().adx_tconv_plan_describe(C.byref(desc), batch, scratch_floats, int(tickets), C.byref(n), ints, 4),
            "adx_tconv_plan_describe")
    return _records(ints, n.value)


def layer_key(r):
    """Which layer a record belongs to: the (first) conv of the launch; the reduce launch behind a split and the launches without
    weights are layers of their own."""
    return (r["group"], r["block"], r["conv"], "reduce" if r["family"] == "reduce" else r["aux"])


def signature(r):
    return tuple(r[k] for k in SIGNATURE)


def describe(r, group_names=None):
    g = group_names[r["group"]] if group_names else f"group{r['group']}"
    s = f"{g}/{'-' if r['block'] < 0 else r['block']}/{CONVS[r['conv']]}"
    if r["conv_b"] >= 0:
        s += f"+{CONVS[r['conv_b']]}"
    return (f"{s}: {r['family']} bt={r['bt']} tiles={r['row_tiles']}x{r['ctiles']}{'+' + str(r['ctiles_b']) if r['ctiles_b'] else ''} "
            f"rows%bt={r['rows_mod_bt']} grid={r['grid']} ksplit={r['ksplit']} reduce={r['reduce']} chunks={r['chunks']} ck={r['ck']} "
            f"vec={r['vec_stage']} fast_epi={r['fast_epi']} taps={r['ntap']}")


def plans(handle, r_max=R_MAX, flags=ASSUME_PACKED):
    """{rows: records} for rows 1..r_max."""
    return {rows: plan(handle, rows, flags) for rows in range(1, r_max + 1)}


def signature_table(all_plans):
    """{layer: {rows: (signature, rows % bt) or None}} over the rows of `all_plans` (None: no launch of that layer at that size, e.g.
    a residual conv that went into its block's pair launch)."""
    layers = {}
    for rows, recs in all_plans.items():
        for r in recs:
            k = layer_key(r)
            assert rows not in layers.setdefault(k, {}), (k, rows)          # one launch per layer and forward
            layers[k][rows] = (signature(r), r["rows_mod_bt"])
    return layers


def runs_of(by_rows, all_rows):
    """Maximal runs of consecutive row counts with one signature: [(signature or None, [rows...])]."""
    out = []
    for rows in all_rows:
        sig = by_rows[rows][0] if rows in by_rows else None
        if out and out[-1][0] == sig:
            out[-1][1].append(rows)
        else:
            out.append((sig, [rows]))
    return out


def plan_cases(all_plans, with_tails=True):
    """The row counts to run: for every layer, every maximal run of consecutive rows with one per-launch signature gives its first
    and its last row count and -- with_tails -- where the run has one, a row count with rows % bt != 0 (a partial last row tile) and one
    with rows % bt == 0.  Nothing is dropped; `with_tails=False` is the boundary-only list of the configurations that do not run
    in full.  Returns the sorted row counts."""
    all_rows = sorted(all_plans)
    table = signature_table(all_plans)
    # a tail case that an earlier layer already put on the list serves later layers too: prefer it (keeps the union small without
    # dropping any (layer, run, kind))
    chosen = set()
    for by_rows in table.values():
        for sig, rr in runs_of(by_rows, all_rows):
            chosen.update((rr[0], rr[-1]))
    if with_tails:
        for by_rows in table.values():
            for sig, rr in runs_of(by_rows, all_rows):
                if sig is None:
                    continue
                for ragged in (True, False):
                    have = [r for r in rr if (by_rows[r][1] != 0) == ragged]
                    if have and not any(r in chosen for r in have):
                        chosen.add(have[0])
    return sorted(chosen)


def coverage(all_plans, cases):
    """(distinct (layer, signature) pairs in all_plans, those of them that `cases` reach)."""
    table = signature_table(all_plans)
    every, reached = set(), set()
    for k, by_rows in table.items():
        for rows, (sig, _) in by_rows.items():
            every.add((k, sig))
            if rows in cases:
                reached.add((k, sig))
    return every, reached


def tail_samples(recs, rows):
    """Indices of the samples that sit in a partial last row tile of some launch of this forward (rows % bt != 0 there)."""
    tail = set()
    for r in recs:
        if r["family"] in TILED and r["rows_mod_bt"] != 0:
            tail.update(range(rows - r["rows_mod_bt"], rows))
    return sorted(tail)
