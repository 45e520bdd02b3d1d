"""Cell-layout launches of conv2d_hs3x3q_kernel on small shapes whose unit walk changes cout tile mid-walk, has uneven XCD ranges and
padding workgroups, plus one perception pass -- in a process of its own, so that switches read once per process (ADX_HS_PERSIST,
ADX_HS_RESERVE_CUS, ADX_HS_GRID_CAP, ADX_RESNET_STREAMS) can be set for it.  usage: python tests/hs3x3q_walk_worker.py OUT.pt;
saves {case: tensor}."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# stride 1: (cin, cout, batch, h, w) -- 6 x 2, 2 x 4 and 21 x 1 (spatial tiles x cout tiles) units over 8 XCDs: ranges of one and
# two units, of one unit each, of two and three, and -- three cout tiles, 45 units -- of five and six, walked to the end by ONE
# workgroup per XCD under ADX_HS_GRID_CAP=8 with the cout tile changing at every step.  (128 -> 128 on 17 x 33 maps takes six
# images: with three the launch is a split reduction of the 32x32x16 kernel, which has no cell form -- conv2d_hs3x3_plan: split_shape.)
CONVS = ((64, 256, 3, 9, 29), (64, 512, 2, 8, 29), (128, 128, 6, 17, 33), (64, 384, 5, 17, 29))
# block entries: (cin, cout, batch, h, w) of the INPUT -- outputs of 9 x 17: 4 x 1 and 4 x 2 units at three images (no range
# longer than one unit on any grid), 10 x 1 and 10 x 2 at eight: ranges of one and two, of two and three units, which ONE workgroup
# per XCD walks under ADX_HS_GRID_CAP=8 -- the cout tile of 128 -> 256 changing at every step (the next unit's first tap, the reload
# of conv1's and the downsample's constants)
ENTRIES = ((64, 128, 3, 17, 33), (128, 256, 3, 17, 33), (64, 128, 8, 17, 33), (128, 256, 8, 17, 33))
PERCEPTION = (32, 64, 96)


def outputs():
    from autonomous_driving_with_diffusion_model_amd import ops
    from autonomous_driving_with_diffusion_model_amd.modeling.perception import PerceptionResNet34
    from autonomous_driving_with_diffusion_model_amd.utils import procedural as P
    dev = "cuda:0"
    out = {}
    for cin, cout, b, h, w in CONVS:
        g = torch.Generator(device="cpu").manual_seed(cin * 7 + cout + b)
        x = torch.randn((b, cin, h, w), generator=g).to(dev)
        wt = (torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (cin * 9)) ** 0.5).to(dev)
        sc, sh = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.1).to(dev)
        res = ops.to_cells(torch.randn((b, cout, h, w), generator=g).to(dev))
        _, packed = ops.conv2d(x[:1], wt, stride=1, pad=1)
        for with_res in (False, True):
            y = ops.conv2d_cells(ops.to_cells(x), packed, cin, cout, b, h, w, x_cells=True, scale=sc, shift=sh,
                                 res=res if with_res else None, res_cells=with_res, relu=True)
            out[f"conv {cin}x{cout}b{b}@{h}x{w} res={int(with_res)}"] = y.cpu()
    for cin, cout, b, h, w in ENTRIES:
        g = torch.Generator(device="cpu").manual_seed(cin * 5 + cout + b)
        x = torch.randn((b, cin, h, w), generator=g).to(dev)
        w1 = (torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (cin * 9)) ** 0.5).to(dev)
        wd = (torch.randn((cout, cin, 1, 1), generator=g) * (1.0 / cin) ** 0.5).to(dev)
        c = [(torch.rand(cout, generator=g) + 0.5).to(dev) if i % 2 == 0 else (torch.randn(cout, generator=g) * 0.1).to(dev) for i in range(4)]
        y1, yd, _ = ops.conv2d_block_s2_cells(ops.to_cells(x), w1, wd, b, h, w, scale1=c[0], shift1=c[1], scaled=c[2], shiftd=c[3])
        out[f"entry {cin}x{cout}b{b}@{h}x{w} conv1"] = y1.cpu()
        out[f"entry {cin}x{cout}b{b}@{h}x{w} downsample"] = yd.cpu()
    m = PerceptionResNet34(64)
    P.load_procedural(m, 0)
    m = m.to(dev).eval()
    b, h, w = PERCEPTION
    img = torch.randn((b, 3, h, w), generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        out["perception"] = m(img).float().cpu()
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    torch.save(outputs(), sys.argv[1])
