"""What the conv host code answers over a grid of layer descriptors, as JSON (dev tool; needs the built library, no GPU).

    python tools/dev/conv_host_dump.py OUT.json

For every descriptor of the grid: ft_conv_pack_geometry (status + fields), ft_conv_tile_candidates (count or negative status + the
hints, max 64), ft_conv_workspace_bytes, ft_conv_shift_nstride_supported and ft_conv_flops, in a fixed order.  Two trees validate,
pack, enumerate tiles and size workspaces alike exactly when their dumps are byte-equal; run it from each tree (it loads the library
of the tree it lies in).  A descriptor the library rejects is recorded with its status, not skipped.
Grid: fp16 / fp32; Cin 3, 6, 12 (row-packed, 4 / 8 / 16 channels per pixel) and 24 .. 2048; Cout 2 .. 2048; 1x1 s1 / s2, 3x3 s1 / s2,
5x5 s2, 7x7 s2 and the transposed 4x4; six (N, H, W); each plain and with one of has_residual, x2_cin, tail_cout = 17, pool,
shift_nstride, NCHW output."""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowtrack.pytorch_amd import _lib
from flowtrack.pytorch_amd._lib import ConvDesc, ConvGeometry

CINS = [(3, 4), (6, 8), (12, 16)] + [(c, 0) for c in (24, 64, 96, 128, 256, 512, 1024, 2048)]     # (Cin, row-packed x_cstride or 0)
COUTS = [2, 4, 17, 32, 64, 128, 192, 256, 512, 1024, 2048]
FORMS = [("1x1s1", 1, 1, 0, 0), ("1x1s2", 1, 2, 0, 0), ("3x3s1", 3, 1, 1, 0), ("3x3s2", 3, 2, 1, 0), ("5x5s2", 5, 2, 2, 0), ("7x7s2", 7, 2, 3, 0),
         ("t4x4", 4, 2, 1, 1)]                                                                    # (name, k, stride, pad, transposed)
SHAPES = [(1, 8, 6), (2, 17, 13), (8, 32, 24), (64, 64, 48), (64, 8, 6), (16, 6, 8)]
FLAGS = ["plain", "residual", "x2", "tail", "pool", "shift_n", "nchw"]


def round_up(x, m):
    return (x + m - 1) // m * m


def desc(dtype, cin, rowc, cout, form, shape, flag):
    _, k, s, p, tr = form
    N, H, W = shape
    d = ConvDesc()
    d.dtype, d.N, d.Hi, d.Wi, d.Cin, d.Cout = dtype, N, H, W, cin, cout
    d.kh = d.kw = k
    d.stride, d.pad, d.transposed = s, p, tr
    d.Ho, d.Wo = (2 * H, 2 * W) if tr else ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)
    if rowc:
        d.x_cstride = rowc
        d.x_lpad = p + 2 if flag == "pool" else p
        d.x_wpitch = d.x_lpad + W + p
    else:
        d.x_cstride = round_up(cin, 32)
    d.out_layout = _lib.FT_LAYOUT_NCHW_F32 if flag == "nchw" else _lib.FT_LAYOUT_NHWC
    d.y_cstride = 0 if flag == "nchw" else round_up(17 if flag == "tail" else cout, 8)
    d.act = _lib.FT_ACT_RELU
    if flag == "residual":
        d.has_residual, d.res_cstride = 1, round_up(cout, 8)
    elif flag == "x2":
        d.x2_cin, d.x2_hi, d.x2_wi, d.x2_cstride, d.x2_stride = 64, d.Ho, d.Wo, 64, 1
    elif flag == "tail":
        d.tail_cout = 17
    elif flag == "pool":
        d.pool = 1
    elif flag == "shift_n":
        d.shift_nstride = round_up(cout, 4)
    return d


def main(out):
    lib = _lib.load()
    hints = (ctypes.c_int * 64)()
    rows = []
    for dtype in (_lib.FT_F16, _lib.FT_F32):
        for cin, rowc in CINS:
            for cout in COUTS:
                for form in FORMS:
                    for shape in SHAPES:
                        for flag in FLAGS:
                            d = desc(dtype, cin, rowc, cout, form, shape, flag)
                            g = ConvGeometry()
                            st = lib.ft_conv_pack_geometry(ctypes.byref(d), ctypes.byref(g))
                            n = lib.ft_conv_tile_candidates(ctypes.byref(d), hints, 64)
                            rows.append({
                                "desc": f"{'f16' if dtype == _lib.FT_F16 else 'f32'} cin{cin} cout{cout} {form[0]} n{shape[0]} {shape[1]}x{shape[2]} {flag}",
                                "geometry": [st] + (list(g.key()) if st == 0 else []),
                                "candidates": [n] + [int(h) for h in hints[:max(n, 0)]],
                                "workspace": int(lib.ft_conv_workspace_bytes(ctypes.byref(d))),
                                "shift_nstride": lib.ft_conv_shift_nstride_supported(ctypes.byref(d)),
                                "flops": float(lib.ft_conv_flops(ctypes.byref(d))),
                            })
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} descriptors -> {out}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
