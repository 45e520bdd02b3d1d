"""The per-process half of tests/test_gpu_pipe_handoff.py: switches read once per process (ADX_UNET_PIPE=0: the deepest level as
launches; ADX_UNET_CHAIN=0: no chained level opens a forward) need a process of their own.
Usage: python tests/pipe_handoff_worker.py outputs OUT.pt   -- every case's first forwards, and whether they took the pipeline
       python tests/pipe_handoff_worker.py epochs OUT.json  -- forward-number increments per conditioning path"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import pipe_layout  # noqa: E402
import test_gpu_pipe_handoff as T  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]
if mode == "outputs":
    res = {}
    for case in T.CASES:
        _, _, outs, runs = T.first_outputs(case, check_runs=False)
        res[case[0]] = {"runs": runs, "outs": outs}
    torch.save(res, out)
elif mode == "epochs":
    case = T.CASES[T.CASE_IDS.index("free_h16_pair")]
    m, inputs = T.case_model(case, check_runs=False)
    res = {"runs": pipe_layout(m._native(), case[3])["runs"]}
    for path in ("per_step", "precomputed"):
        res[path] = T._deltas(m, inputs[0], path == "precomputed")
    with open(out, "w") as f:
        json.dump(res, f)
else:
    raise SystemExit(f"unknown mode {mode}")
