"""Fixed cost of a launch of the fp32 gconv kernel ("Fixed cost of a tile"): single-launch times of a
64 x 64-tile GEMM with ONE k-tile per block and each epilogue flavour, and of the 128 x 32 data gradient of D's second
conv at B = 512 (HIP events around N back-to-back launches, best of five): python scratch/mb_fixed_cost.py [tag]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "imagecfgen-pytorch_amd")]
import torch
from ali_hip import ops

N = 400
dev = "cuda"


def timeit(name, fn):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / N * 1e3)
    print(f"{name:46s} {best:8.2f} us", flush=True)
    return best


tag = sys.argv[1] if len(sys.argv) > 1 else ""
print("== fixed cost", tag, {k: v for k, v in os.environ.items() if k.startswith("ALI_")})
tiny = torch.zeros(64, device=dev)
timeit("floor: 64-element fill", lambda: tiny.fill_(1.0))

with ops.tuning(ALI_BM=64, ALI_BN=64):
    for HW in (8, 16):           # 512 / 2048 tiles of 64 x 64: 2 and 8 per CU
        B, C, K = 512, 32, 64
        x = torch.randn(B, HW, HW, C, device=dev)
        w = (torch.randn(K, 1, C, device=dev) * 0.1).contiguous()
        y = torch.empty(B, HW, HW, K, device=dev)
        g = ops.geom(B, HW, HW, C, HW, HW, K, 1, 1, 1, 0)
        mask = (torch.rand(B, K, device=dev) > 0.5).float() * 2
        yprev = torch.randn(B, HW, HW, K, device=dev)
        bias = torch.randn(K, device=dev)
        e_none = ops.epilogue()
        e_bias = ops.epilogue(bias=bias, act=ops.ACT_LEAKY, slope=0.1)
        e_mask = ops.epilogue(bias=bias, act=ops.ACT_LEAKY, slope=0.1, mask=mask)
        e_md = ops.epilogue(mask=mask, dact_y=yprev, dact=ops.ACT_LEAKY, dslope=0.1)
        timeit(f"1-ktile 64x64 {HW}x{HW} no operands", lambda: ops.conv_fwd(g, x, w, y, e_none))
        timeit(f"1-ktile 64x64 {HW}x{HW} bias+leaky", lambda: ops.conv_fwd(g, x, w, y, e_bias))
        timeit(f"1-ktile 64x64 {HW}x{HW} bias+leaky+mask", lambda: ops.conv_fwd(g, x, w, y, e_mask))
        timeit(f"1-ktile 64x64 {HW}x{HW} mask+dact_y", lambda: ops.conv_fwd(g, x, w, y, e_md))
        # bn_mode 2: data gradient of a 1x1 conv K2 -> C2 (output has 64 channels)
        g2 = ops.geom(B, HW, HW, K, HW, HW, C, 1, 1, 1, 0)
        gy = torch.randn(B, HW, HW, C, device=dev)
        wd = (torch.randn(K, 1, C, device=dev) * 0.1).contiguous()
        slots = ops.conv_mtiles(g2, 1)[0]
        part = torch.zeros(2 * K * slots, device=dev)
        mean, invstd = torch.randn(K, device=dev), torch.rand(K, device=dev) + 0.5
        e_bn2 = ops.epilogue(bn_bwd=(part, yprev, mean, invstd, mask, mask, slots))
        timeit(f"1-ktile 64x64 {HW}x{HW} bn_mode 2 (two masks)", lambda: ops.conv_bwd_data(g2, gy, wd, y, e_bn2))

# the 128 x 32 data gradient of D's second conv (32 -> 64, 4 x 4 stride 2, 24 x 24 -> 11 x 11), B = 512, bn_mode 2
B = 512
g3 = ops.geom(B, 24, 24, 32, 11, 11, 64, 4, 4, 2, 0)
gy = torch.randn(B, 11, 11, 64, device=dev)
wd = (torch.randn(32, 16, 64, device=dev) * 0.05).contiguous()
dx = torch.empty(B, 24, 24, 32, device=dev)
xin = torch.randn(B, 24, 24, 32, device=dev)
slots, rows, pm = ops.conv_mtiles(g3, 1)
print("D conv2 dgrad: slots", slots, "tile rows", rows, "pixel-major", pm)
part = torch.zeros(2 * 32 * slots, device=dev)
mean, invstd = torch.randn(32, device=dev), torch.rand(32, device=dev) + 0.5
m_in = (torch.rand(B, 32, device=dev) > 0.2).float() * 1.25
e3 = ops.epilogue(bn_bwd=(part, xin, mean, invstd, m_in, m_in, slots))
e3n = ops.epilogue()
timeit("D conv2 dgrad 128x32 bn_mode 2", lambda: ops.conv_bwd_data(g3, gy, wd, dx, e3))
timeit("D conv2 dgrad 128x32 no operands", lambda: ops.conv_bwd_data(g3, gy, wd, dx, e3n))
