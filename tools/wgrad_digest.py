#!/usr/bin/env python3
"""sha256 of what orehip.conv2d_wgrad writes, case by case: the yardstick of a refactor of the weight-gradient kernels that must not
change a bit.

    python tools/wgrad_digest.py > digest.txt        (once in a tree of the parent commit, once in the new tree; the files must be equal)

The cases are the shapes and seeded operands of tests/wgrad_ref.py, in fp32 and in bf16 mode: every shape of MATRIX with and without the
bias gradient, beta = 0 and beta = 1 into seeded old values; CAP_SHAPE under every workspace of CAPS (S = 1, 2, 3, 17 through the C
ABI) for k = 1 and 3.  One line per case: the sha256 of the dW bytes and of the db bytes ("-" without a bias gradient).  Operands and
old values are drawn on the CPU, so the lines depend on the library alone."""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "faster-orefsdet_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import wgrad_ref as WR  # noqa: E402


def sha(t):
    return "-" if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    import orehip as oh
    P = C.c_void_p
    for mode in ("fp32", "bf16"):
        prev = oh.set_conv_precision(mode)
        for (B, H, W, Cin, Cout, k) in WR.MATRIX:
            M = B * H * W
            x, dz = WR.scaled_operands(B, H, W, Cin, Cout, seed=M + 7 * Cin + Cout + k)
            g = torch.Generator().manual_seed(M + k)
            old_w, old_b = torch.randn(Cout, Cin, k, k, generator=g), torch.randn(Cout, generator=g)
            xd, zd = x.cuda(), dz.cuda()
            for bias in (False, True):
                for beta in (0.0, 1.0):
                    dw, db = old_w.cuda(), (old_b.cuda() if bias else None)
                    kw = dict(want_bias=True, db_out=db, beta_b=beta) if bias else {}
                    oh.conv2d_wgrad(xd, zd, k, out=dw, beta=beta, **kw)
                    print(f"{mode} matrix {B},{H},{W},{Cin},{Cout},{k} bias={int(bias)} beta={beta:g} dW {sha(dw)} db {sha(db)}")
        B, H, W, Cin, Cout = WR.CAP_SHAPE
        for k in (1, 3):
            per = WR.slab_floats(Cin, Cout, k)
            for cap in WR.CAPS:
                n = cap * per + per // 2
                x, dz = WR.scaled_operands(B, H, W, Cin, Cout, seed=100 + cap + k)
                xd, zd = x.cuda(), dz.cuda()
                ws = torch.empty(n, device="cuda")
                dw, db = torch.empty(Cout, Cin, k, k, device="cuda"), torch.empty(Cout, device="cuda")
                rc = oh.lib().ore_conv2d_wgrad_bias_fwd(P(xd.data_ptr()), Cin, 0, P(zd.data_ptr()), Cout, 0, B, H, W, Cin, Cout, k, k, k // 2,
                                                        P(dw.data_ptr()), C.c_float(0.0), P(db.data_ptr()), C.c_float(0.0), P(ws.data_ptr()),
                                                        C.c_size_t(n), oh._stream())
                assert rc == 0, oh.lib().ore_last_error().decode()
                print(f"{mode} cap {B},{H},{W},{Cin},{Cout},{k} S={cap} dW {sha(dw)} db {sha(db)}")
        oh.set_conv_precision(prev)


if __name__ == "__main__":
    main()
