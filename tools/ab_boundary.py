"""The two fp32-tensor boundary kernels of this tree's library against another build of the same ABI (e.g. one linked with an older
elementwise.hip), bit for bit: `python tools/ab_boundary.py path/to/other/libunirestore_hip.so` on an MI355X (profiles/restore_io.txt, 5)."""
import ctypes as C, os, sys, itertools
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unirestore_amd import capi
new = capi.lib
old = C.CDLL(os.path.abspath(sys.argv[1]))
for n in ("ur_image_resize_pad_nhwc", "ur_image_unpad_resize_nchw"):
    getattr(old, n).restype, getattr(old, n).argtypes = capi.SIGNATURES[n]
g = torch.Generator().manual_seed(0)
bad = 0
cases = [(37, 53, 90, 131, 6, 29), (64, 96, 40, 60, 24, 4), (48, 48, 48, 48, 16, 16), (96, 80, 614, 512, 26, 0), (300, 500, 512, 853, 0, 43),
         (100, 84, 610, 512, 30, 0), (70, 70, 512, 512, 0, 0), (511, 700, 512, 701, 0, 3), (256, 256, 512, 512, 0, 0)]
for dt, tdt in ((0, torch.bfloat16), (1, torch.float16)):
    for (h, w, rh, rw, ph, pw) in cases:
        img = torch.rand(2, 3, h, w, generator=g).cuda()
        outs = []
        for lib in (old, new):
            y = torch.empty(2, rh + ph, rw + pw, 8, dtype=tdt, device="cuda")
            rc = lib.ur_image_resize_pad_nhwc(img.data_ptr(), y.data_ptr(), 2, 3, h, w, rh, rw, ph, pw, 8, 2.0, -1.0, dt, None)
            assert rc == 0
            outs.append(y)
        torch.cuda.synchronize()
        eq = torch.equal(outs[0], outs[1]); bad += not eq
        print("resize_pad", dt, (h, w, rh, rw, ph, pw), "equal" if eq else "DIFFERENT")
        for f32, q in itertools.product((1, 0), (0, 1)):
            x = (torch.randn(2, rh + ph, rw + pw, 8, generator=g) * 0.6).cuda()
            x = x if f32 else x.to(tdt)
            outs = []
            for lib in (old, new):
                o = torch.empty(2, 3, h, w, device="cuda")
                rc = lib.ur_image_unpad_resize_nchw(x.data_ptr(), f32, o.data_ptr(), 2, 3, rh + ph, rw + pw, 8, rh, rw, h, w, 0.5, 0.5, q, dt, None)
                assert rc == 0
                outs.append(o)
            torch.cuda.synchronize()
            eq = torch.equal(outs[0], outs[1]); bad += not eq
            print("unpad_resize", dt, f32, q, (h, w), "equal" if eq else "DIFFERENT")
print("outputs that differ:", bad)
sys.exit(1 if bad else 0)
