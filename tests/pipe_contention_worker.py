"""One of several processes that sample on the SAME GPU at the same time (tests/test_gpu_callers.py): one scene, H = 16,
classifier-free guidance -- the configuration whose deepest level runs as the pipeline launch (csrc/tconv_pipe.hip: 225 workgroups,
one per CU, later stages spinning on earlier ones).  With another process holding CUs the pipeline's workgroups cannot all be
resident at once; the launch must still complete (a stage waits only for workgroups dispatched before it) and give the same bits.
The graph ticks cycle through three inputs, each checked against its own eager reference.
Usage: python tests/pipe_contention_worker.py OUT TICKS"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from autonomous_driving_with_diffusion_model_amd import scheduler as S  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.sampling import GraphedSampler, generate_traj  # noqa: E402
from autonomous_driving_with_diffusion_model_amd.utils import procedural as P  # noqa: E402
from helpers import SCHED_KW  # noqa: E402
from test_gpu_model import make_model  # noqa: E402

DEV = "cuda:0"
out, ticks = sys.argv[1], int(sys.argv[2])
m, cfg = make_model("FREE_GUIDANCE", 16)
cfg.EVAL.SAMPLE_STEPS, cfg.GUIDANCE.FREE_SCALE = 20, 7.5
sch = S.GuidanceDDIMScheduler(cfg=cfg, thresholding=True, **SCHED_KW)
# three seeded inputs (camera frame, target, initial trajectory): the ticks cycle through them, so a tick that read what the tick
# before it left in the pipeline's records or block outputs would show up as another input's bits
ds = [{k: v.to(DEV) for k, v in P.synthetic_batch(1, 16, image_hw=(64, 96), seed=s).items()} for s in (5, 6, 7)]
res = []
with torch.no_grad():
    refs = [generate_traj(m, sch, cfg, d["imgs"], d["target"], d["init_trajs"]) for d in ds]
    gs = GraphedSampler(m, sch, cfg)
    for i in range(ticks):
        d = ds[i % 3]
        res.append((i % 3, gs(d["imgs"], d["target"], d["init_trajs"]).clone()))
torch.cuda.synchronize()
same = all(torch.equal(r, refs[k]) for k, r in res)
mismatch = [i for i, (k, r) in enumerate(res) if not torch.equal(r, refs[k])]
torch.save({"first": refs[0].cpu(), "refs": [r.cpu() for r in refs], "all_equal": bool(same), "mismatched_ticks": mismatch,
            "finite": bool(all(torch.isfinite(r).all() for r in refs)),
            "distinct": bool(not torch.equal(refs[0], refs[1]) and not torch.equal(refs[1], refs[2]))}, out)
