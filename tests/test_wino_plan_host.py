"""CPU: the planner keeps the Winograd kernels inside what their buffer descriptors can address.  The kernels read every image through
a descriptor whose num_records is the image's size in bytes, and mark a column outside the image with the offset 2^31: an image of 2^31
bytes or more must not be planned on them (the layer takes a direct kernel, as it does below the row thresholds); one image row less
must.  Fake pointers, no GPU."""
import os

import pytest


@pytest.fixture(scope="module")
def ore():
    import orehip
    if not os.path.exists(orehip.LIB_PATH):
        orehip.build()
    orehip.lib()
    return orehip


def _desc(ore, H, W, Cin, Cout, ld):
    d = ore.ConvDesc()
    d.in_, d.w, d.out, d.w_wino, d.workspace = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    d.in_ld, d.in_coff, d.B, d.H, d.W, d.Cin = ld, 0, 1, H, W, Cin
    d.Cout, d.kh, d.kw, d.stride, d.pad = Cout, 3, 3, 1, 1
    d.out_ld, d.out_coff, d.workspace_floats = Cout, 0, 1 << 24
    return d


@pytest.mark.parametrize("Cin,Cout,ld,W", [(64, 64, 64, 4096), (128, 128, 128, 2048), (80, 80, 352, 1024), (112, 112, 128, 4096)])
def test_image_of_2_to_31_bytes_is_not_winograd(ore, Cin, Cout, ld, W):
    wino = (ore.CONV_LAUNCHERS.index("k_conv3x3_wino"), ore.CONV_LAUNCHERS.index("k_conv3x3_wino_nu"))
    H = -(-(1 << 31) // (W * ld * 4))                   # the first height at which the image reaches 2^31 bytes
    assert H * W * ld * 4 >= 1 << 31 > (H - 1) * W * ld * 4
    try:
        for mode in (1, 2):                             # automatic and forced
            assert ore.lib().ore_conv_set_plan_override(-7, mode, 0, 0, 0) == 0
            big = ore.conv_plan(_desc(ore, H, W, Cin, Cout, ld))
            assert big.launcher not in wino and big.launcher != 0, ore.CONV_LAUNCHERS[big.launcher]
            small = ore.conv_plan(_desc(ore, H - 1, W, Cin, Cout, ld))
            assert small.launcher == wino[0 if Cin in (64, 128) else 1], ore.CONV_LAUNCHERS[small.launcher]
    finally:
        ore.lib().ore_conv_reset_plan_overrides()
