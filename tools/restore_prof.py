"""The four boundary kernels at B = 8, 512 x 512 and at a resizing geometry (profiles/restore_io.txt):
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/restore_prof.py` on an MI355X."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from unirestore_amd import ops
ops.set_dtype("bf16")
g = torch.Generator().manual_seed(0)
for (h, w, rh, rw, ph, pw) in [(512, 512, 512, 512, 0, 0), (300, 500, 512, 853, 0, 43)]:
    ch, cw = rh + ph, rw + pw
    u8 = torch.randint(0, 256, (8, h, w, 3), generator=g, dtype=torch.uint8)
    slots = torch.zeros(8, ch * cw * 3, dtype=torch.uint8)
    slots[:, :h * w * 3] = u8.reshape(8, -1)
    slots = slots.cuda()
    geom = ops.ragged_geometry([(h, w, rh, rw)] * 8, (ch, cw)).cuda()
    f32 = (u8.permute(0, 3, 1, 2).float() / 255).contiguous().cuda()
    x = (torch.randn(8, ch, cw, 8, generator=g) * 0.6).cuda()
    for _ in range(10):
        a = ops.image_u8_ingest(slots, geom, (ch, cw), validate=False)
        b = ops.image_resize_pad(f32, rh, rw, ph, pw)
        c, _ = ops.image_u8_egress(x, 3, geom, mul=0.5, add=0.5, validate=False)
        d = ops.image_unpad_resize(x, 3, (rh, rw), (h, w), mul=0.5, add=0.5, quantize=True)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
