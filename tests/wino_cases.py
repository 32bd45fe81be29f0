"""The Winograd launch forms that tests/test_hip_wino_desc.py pins and tools/gen_wino_parent_hashes.py records: the smallest shapes at
which descriptor addressing of the input can go wrong (row / column wrap-around, tiles hanging over the edges, the boundary between two
images and between two pyramid levels, channel slices of wider buffers), over all five builds.  Inputs are seeded on the CPU; run()
launches one case with the Winograd kernel forced by the caller and returns the whole output buffer, sentinel included."""
import hashlib

import torch
import torch.nn.functional as F

BUILDS = (64, 128, 80, 96, 112)                    # k_conv3x3_wino<64 | 128>, k_conv3x3_wino_nu<80 | 96 | 112>
SENTINEL = 7.0
GUARD_PIXELS = 64                                  # NaN pixels in front of and behind the tensor in the guarded form

SINGLE = ((1, 2, 2), (1, 5, 1), (1, 1, 7),         # (B, H, W): row / column wrap-around
          (2, 13, 11), (1, 9, 33), (3, 3, 5))      # no multiple of the 4 x 16 batch; two and three images
LEVELS = (((5, 7), (3, 4), (2, 2)), ((12, 20), (6, 10), (3, 5)))      # three levels in one launch, B = 2
SLICES = ((64, 192, (64, 128)), (112, 352, (80, 96, 112)))            # (in_coff, ld, builds), B = 2, 13 x 11


def cout_of(cin):
    return 64 if cin in (64, 128) else cin


def _cases():
    out = []
    for cin in BUILDS:
        for B, H, W in SINGLE:
            out.append(dict(id=f"c{cin}-b{B}-{H}x{W}", kind="single", cin=cin, B=B, HW=((H, W),), in_coff=0, ld=cin, multi=B > 1))
        for HW in LEVELS:
            out.append(dict(id=f"c{cin}-tower-{HW[0][0]}x{HW[0][1]}", kind="tower", cin=cin, B=2, HW=HW, in_coff=0, ld=cin, multi=True))
            if cin in (64, 128):
                out.append(dict(id=f"c{cin}-fpn-{HW[0][0]}x{HW[0][1]}", kind="fpn", cin=cin, B=2, HW=HW, in_coff=0, ld=cin, multi=True))
    for coff, ld, builds in SLICES:
        for cin in builds:
            out.append(dict(id=f"c{cin}-slice{coff}of{ld}", kind="single", cin=cin, B=2, HW=((13, 11),), in_coff=coff, ld=ld, multi=True))
    return out


CASES = _cases()
GUARDED = [c for c in CASES if c["multi"]]         # the slice and multi-image cases


def make(case):
    """Seeded CPU data of a case: xs[l] [B, ld, H_l, W_l] (the whole buffer, slice included), ws[j] / sc / sh[j] per weight set."""
    cin, cout = case["cin"], cout_of(case["cin"])
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(case["id"])))
    xs = [torch.randn(case["B"], case["ld"], h, w, generator=g) for h, w in case["HW"]]
    nw = len(case["HW"]) if case["kind"] == "fpn" else 1
    ws = [torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5 for _ in range(nw)]
    sc = torch.rand(cout, generator=g) + 0.5
    sh = [torch.randn(cout, generator=g) * 0.1 for _ in range(nw)]
    return xs, ws, sc, sh


def out_geometry(case):
    """(out_ld, out_coff): slice cases write into a wider buffer too."""
    cout = cout_of(case["cin"])
    return (cout + 96, 32) if case["in_coff"] else (cout + 8, 4)


def reference(case, data):
    """float64 F.conv2d + epilogue per level, rows [sum_l B * H_l * W_l, Cout] level-major."""
    xs, ws, sc, sh = data
    cin, c0 = case["cin"], case["in_coff"]
    rows = []
    for l, x in enumerate(xs):
        j = l if case["kind"] == "fpn" else 0
        y = F.conv2d(x[:, c0:c0 + cin].double(), ws[j].double(), None, 1, 1)
        if case["kind"] != "fpn":
            y = y * sc.double().view(1, -1, 1, 1)
        y = y + sh[j].double().view(1, -1, 1, 1)
        if case["kind"] == "single":
            y = F.relu(y)
        rows.append(y.permute(0, 2, 3, 1).reshape(-1, y.shape[1]))
    return torch.cat(rows, 0)


def run(ore, case, data, guarded=False):
    """One launch of the case (single: FrozenBN scale / shift + ReLU; tower: shared weights, scale / shift; fpn: per-level weights and
    bias).  Returns the output rows [rows, out_ld] on the CPU.  guarded: the input lives inside a larger allocation whose pixels in front
    of and behind the tensor, and whose channels outside the slice, are NaN."""
    xs, ws, sc, sh = data
    cin, cout, c0, ld, B = case["cin"], cout_of(case["cin"]), case["in_coff"], case["ld"], case["B"]
    rows = torch.cat([x.permute(0, 2, 3, 1).reshape(-1, ld) for x in xs], 0).contiguous()
    if guarded:
        rows = rows.clone()
        keep = torch.zeros(ld, dtype=torch.bool)
        keep[c0:c0 + cin] = True
        rows[:, ~keep] = float("nan")
        big = torch.full((rows.shape[0] + 2 * GUARD_PIXELS, ld), float("nan"))
        big[GUARD_PIXELS:GUARD_PIXELS + rows.shape[0]] = rows
        rows_dev = big.cuda()[GUARD_PIXELS:GUARD_PIXELS + rows.shape[0]]
        assert rows_dev.is_contiguous() and rows_dev.storage_offset() == GUARD_PIXELS * ld
    else:
        rows_dev = rows.cuda()
    out_ld, out_coff = out_geometry(case)
    out = torch.full((rows.shape[0], out_ld), SENTINEL).cuda()
    wps = [ore.pack_conv_weight(w).cuda() for w in ws]
    Us = [ore.winograd_weight(wp, cout, cin) for wp in wps]
    if case["kind"] == "single":
        (H, W), = case["HW"]
        ore.conv2d(rows_dev.view(B, H, W, ld), wps[0], cout, 3, 1, in_coff=c0, Cin=cin, scale=sc.cuda(), shift=sh[0].cuda(), relu_cout=cout,
                   out=out.view(B, H, W, out_ld), out_coff=out_coff, w_wino=Us[0])
    elif case["kind"] == "tower":
        ore.conv2d_levels(rows_dev, case["HW"], B, wps[0], cout, 3, in_coff=c0, Cin=cin, scale=sc.cuda(), shift=sh[0].cuda(), out=out,
                          out_coff=out_coff, w_wino=Us[0])
    else:
        U = torch.stack(Us).contiguous()
        ore.conv2d_levels(rows_dev, case["HW"], B, wps[0], cout, 3, in_coff=c0, Cin=cin, shift=torch.stack(sh).contiguous().cuda(),
                          ep_stride=cout, out=out, out_coff=out_coff, w_wino=U, w_wino_level_stride=U.shape[1])
    name = ore.conv_last_launch()[0]
    assert name == ("k_conv3x3_wino" if cin in (64, 128) else "k_conv3x3_wino_nu"), name
    return out.cpu()


def digest(out_rows):
    return hashlib.sha256(out_rows.contiguous().numpy().tobytes()).hexdigest()
