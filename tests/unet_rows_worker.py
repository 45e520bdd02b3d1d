"""Whole UNet forwards at the plan boundaries of THIS process against the fp64 oracle (tests/test_gpu_unet_rows.py), in a process
of its own so that the switches read once per process (ADX_UNET_CHAIN=0, ADX_UNET_PIPE=0) can be set for it.  The plan export
(adx_unet_plan_describe), called here, gives this variant's own row counts.

usage: unet_rows_worker.py H [H ...] [--rows r,r,...]      (--rows: run these row counts instead of the export's)
prints  FORWARD ... (the plan, before each forward)   ERR rows=.. worst=.. tail(n)=.. rest=..
        FAMILIES <comma list>                          kernel families seen over the cases of one horizon
        PLANT <family> <first group reported> <groups>  1e5 planted in the trajectory of the last real sample at 33 rows
        DONE H=.. cases=.. worst=.. failures=N         and the failure texts after it"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import unet_plan as UP  # noqa: E402
from test_gpu_unet_rows import build, hip_forward, inputs, run_cases  # noqa: E402

args = sys.argv[1:]
rows_arg = None
if "--rows" in args:
    i = args.index("--rows")
    rows_arg = [int(v) for v in args[i + 1].split(",")]
    args = args[:i] + args[i + 2:]
rc = 0
for H in (int(a) for a in args):
    dim, mults, use_cond = 64, (1, 2, 4, 8), "FREE_GUIDANCE" if H == 16 else "NO_GUIDANCE"
    m, sd = build(H, dim, mults, use_cond)
    hip_forward(m, *inputs(1, H, dim, use_cond))          # packs: the export is now this process's own plan
    cases = rows_arg or UP.plan_cases(UP.plans(m._native(), UP.R_MAX, flags=0))
    failures, stats = run_cases(m, sd, H, dim, mults, use_cond, cases)
    fams = sorted({r["family"] for rows in cases for r in UP.plan(m._native(), rows, flags=0)})
    print("FAMILIES", ",".join(fams), flush=True)
    rows = 33
    names = [n for n in m.range_group_names() if n.startswith("unet.")]
    reader = [r for r in UP.plan(m._native(), rows, flags=0) if r["group"] == 0 and r["family"] != "aux" and r["conv"] != 7][0]
    x, imgs, t, feat, cond = inputs(rows, H, dim, use_cond)
    x = x.clone()
    x[rows - 1, 5, 1] = 1e5
    m.clear_range_status()
    hip_forward(m, x, imgs, t, feat, cond)
    st = sorted((s for s in m.range_status() if s.startswith("unet.")), key=names.index)
    print("PLANT", reader["family"], st[0] if st else "-", ",".join(st) or "-", flush=True)
    print(f"DONE H={H} cases={len(cases)} worst={max(v[0] for v in stats.values()):.3e} failures={len(failures)}", flush=True)
    for f in failures:
        print(f, flush=True)
    rc |= 1 if failures else 0
sys.exit(rc)
