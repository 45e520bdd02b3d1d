"""A/B two builds of libadx on the SAME GPU: the deployed tick (B = 1, H = 16, 50 steps, one graph).  ADX_LIB selects the library.

    python tools/ab_tick.py libadx_parent.so autonomous_driving_with_diffusion_model_amd/libadx.so
    python tools/ab_tick.py --guided libadx_parent.so autonomous_driving_with_diffusion_model_amd/libadx.so

`--guided`: the 20-step graph ticks of tools/guide_tick_probe.py instead, without a guide and with the largest v1 guide (`none` and
`m32p8i8` at 1 and 64 scenes, three rounds per process): what a change to the guide's routine can move in a tick that does not use it
-- the routeless tick when the route corridor (v4) joined that routine, the capsule-free one when the moving capsules (v5) did."""
import json, os, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
code = "import sys; sys.path.insert(0, %r); import torch, bench, json; print(json.dumps(bench.deployed_leg(torch.device('cuda:0'))))" % root
names = [a for a in sys.argv[1:] if a != "--guided"]
guided = "--guided" in sys.argv[1:]
probe = [sys.executable, os.path.join(root, "tools", "guide_tick_probe.py"), "--arms", "none,m32p8i8", "--rounds", "3"]
for rnd in range(2):
    for name in names:
        env = dict(os.environ, ADX_LIB=os.path.join(root, name))
        out = subprocess.run(probe if guided else [sys.executable, "-c", code], env=env, capture_output=True, text=True)
        line = [l for l in out.stdout.splitlines() if l.startswith("{")]
        if guided and line:
            arms = json.loads(line[-1])["arms"]
            print(rnd, name, json.dumps({k: [v["median_ms"], v["min_ms"], v["max_ms"]] for k, v in arms.items()}), flush=True)
        else:
            print(rnd, name, json.loads(line[-1]).get("tick_ms_graph") if line else out.stderr[-300:], flush=True)
