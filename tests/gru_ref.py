"""The contract of the ConvGRU (include/droid_gru_hip.h) restated in numpy for the tests, generic in the hidden width h
and the input width: the exact fp64 module, the staged contract with its three roundings to half, the per-stage error
bounds, the packed layout and the case tables.  Restated from the header: nothing here imports the package.

Parameters are a dict {layer: (weight, bias)} with the layers convz, convr, convq [h,h+i,3,3], w, convz_glo, convr_glo,
convq_glo [h,h,1,1], biases [h]."""
import numpy as np

import conv3x3_ref as c3

LAYERS = ("convz", "convr", "convq", "w", "convz_glo", "convr_glo", "convq_glo")
GLO = ("convz_glo", "convr_glo", "convq_glo")
U = 2.0 ** -24
# (h, w, B): tests/test_gpu_conv_gru.py says what each one catches; the last two carry the whole step and the gate bound only
MAPS = [(1, 1, 1), (3, 3, 3), (8, 8, 5), (2, 64, 2), (5, 9, 2), (11, 13, 3), (9, 70, 1)]
BIG_MAPS = [(30, 40, 1), (48, 64, 1)]
SPLITS = [(128, 128, 64), (320,)]          # the channels of the inputs after net: inp, corr, flow -- or one tensor


def sigmoid(t):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-t))


def f64(params):
    return {k: (np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)) for k, (w, b) in params.items()}


def halves(params):
    """Every weight and bias rounded to half once: autocast's cast, what the module is packed from."""
    return {k: (np.asarray(w).astype(np.float16), np.asarray(b).astype(np.float16)) for k, (w, b) in params.items()}


def random_params(seed, hidden, inputs, scale=1.0):
    """Seeded fp32 parameters with outputs of order one: 3 x 3 weights ~ N(0, 1 / sqrt(9 C)), 1 x 1 ~ N(0, 1 / sqrt(h))."""
    rng = np.random.default_rng(seed)
    c = hidden + inputs
    out = {}
    for k in LAYERS:
        shape, s = ((hidden, c, 3, 3), 1 / np.sqrt(9 * c)) if k in LAYERS[:3] else ((hidden, hidden, 1, 1), 1 / np.sqrt(hidden))
        out[k] = ((scale * rng.normal(0, s, shape)).astype(np.float32), rng.normal(0, 0.3, (hidden,)).astype(np.float32))
    return out


def operands(seed, splits, h, w, B, hidden=128):
    """net and the inputs after it, half, N(0, 1)."""
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 1, (B, ch, h, w)).astype(np.float16) for ch in (hidden,) + tuple(splits)]


def conv(x, wt):
    """(s, mag) [B,N,H,W] in fp64: sum x w over the zero-padded 3 x 3 windows and sum |x w|; no bias."""
    n = wt.shape[0]
    a = c3.window(np.asarray(x, dtype=np.float64))
    wm = np.asarray(wt, dtype=np.float64).reshape(n, -1).T
    return (a @ wm).transpose(0, 3, 1, 2), (np.abs(a) @ np.abs(wm)).transpose(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------- the exact module
def context(p, net):
    """(g [B,3,h], glo [B,h], a [B,h,H,W], amag) in fp64 from fp64 parameters: g holds both biases of a gate."""
    net = np.asarray(net, dtype=np.float64)
    w1 = p["w"][0].reshape(p["w"][0].shape[0], -1)
    a = np.einsum("nc,bchw->bnhw", w1, net) + p["w"][1][None, :, None, None]
    amag = np.einsum("nc,bchw->bnhw", np.abs(w1), np.abs(net)) + np.abs(p["w"][1])[None, :, None, None]
    glo = (sigmoid(a) * net).mean(axis=(2, 3))
    g = np.stack([glo @ p[k][0].reshape(w1.shape).T + p[k][1] + p[c][1] for k, c in zip(GLO, LAYERS[:3])], axis=1)
    return g, glo, a, amag


def exact(params, net, inputs):
    """The module in fp64: out [B,h,H,W] and the intermediates."""
    p = f64(params)
    net = np.asarray(net, dtype=np.float64)
    inp = np.concatenate([np.asarray(x, dtype=np.float64) for x in inputs], axis=1)
    g = context(p, net)[0]
    x = np.concatenate([net, inp], axis=1)
    z = sigmoid(conv(x, p["convz"][0])[0] + g[:, 0, :, None, None])
    r = sigmoid(conv(x, p["convr"][0])[0] + g[:, 1, :, None, None])
    q = np.tanh(conv(np.concatenate([r * net, inp], axis=1), p["convq"][0])[0] + g[:, 2, :, None, None])
    return dict(out=(1 - z) * net + z * q, z=z, r=r, q=q, g=g)


# ------------------------------------------------------------------------------------------- the stages, each from
# its actual inputs (what the device was given), in fp64 from the HALF parameters, with the bound of the contract's fp32
def stage_context(p16, net16):
    """g in fp64 and its bound.  a is 128 products and a bias summed in fp32 (gamma_130 on sum |w net| + |bw|), sigmoid
    has slope <= 1/4 and an evaluation error of <= 8 u relative (expf, an addition, a division), the product one more
    rounding: 9 u; the mean is P terms and the factor 1 / P: (P + 2) u on mean |sigma net|.  The mat-vec is 128 products
    and two biases, fused or not: gamma_132."""
    p = f64(p16)
    net = np.asarray(net16, dtype=np.float64)
    P = net.shape[2] * net.shape[3]
    g, glo, a, amag = context(p, net)
    sig = sigmoid(a)
    dglo = ((0.25 * 130 * U * amag + 9 * U * sig) * np.abs(net)).mean(axis=(2, 3)) + (P + 2) * U * np.abs(sig * net).mean(axis=(2, 3))
    bounds = []
    for k, c in zip(GLO, LAYERS[:3]):
        wg = np.abs(p[k][0].reshape(g.shape[2], -1))
        bounds.append(dglo @ wg.T + 132 * U * (np.abs(glo) @ wg.T + np.abs(p[k][1]) + np.abs(p[c][1])))
    return g, np.stack(bounds, axis=1)


def _ds(c_in, mag, g):
    return (9 * c_in + 2) * U * (mag + np.abs(g))


def stage_gates(p16, g, net16, inputs16):
    """(z, bound of z16, r * net, bound of rnet16) in fp64 from the device's own g."""
    p = f64(p16)
    net = np.asarray(net16, dtype=np.float64)
    x = np.concatenate([net] + [np.asarray(t, dtype=np.float64) for t in inputs16], axis=1)
    g = np.asarray(g, dtype=np.float64)
    c_in = x.shape[1]
    sz, mz = conv(x, p["convz"][0])
    sr, mr = conv(x, p["convr"][0])
    gz, gr = g[:, 0, :, None, None], g[:, 1, :, None, None]
    z, r = sigmoid(sz + gz), sigmoid(sr + gr)
    bz = 0.25 * _ds(c_in, mz, gz) + 8 * U * z + 2.0 ** -11 * z + 2.0 ** -25
    br = np.abs(net) * (0.25 * _ds(c_in, mr, gr) + 9 * U * r) + 2.0 ** -11 * np.abs(r * net) + 2.0 ** -25
    return z, bz, r * net, br


def stage_update(p16, g, z16, rnet16, net16, inputs16):
    """(out, bound of out16) in fp64 from the device's own g, z16 and rnet16."""
    p = f64(p16)
    net, z = np.asarray(net16, dtype=np.float64), np.asarray(z16, dtype=np.float64)
    x = np.concatenate([np.asarray(t, dtype=np.float64) for t in [rnet16] + list(inputs16)], axis=1)
    gq = np.asarray(g, dtype=np.float64)[:, 2, :, None, None]
    sq, mq = conv(x, p["convq"][0])
    q = np.tanh(sq + gq)
    out = (1 - z) * net + z * q
    bound = z * (_ds(x.shape[1], mq, gq) + 8 * U) + 4 * U * (np.abs(net) + np.abs(q)) + 2.0 ** -11 * np.abs(out) + 2.0 ** -25
    return out, bound


def staged(params, net16, inputs16):
    """The contract end to end in fp64 with its three roundings to half: (g, z16, rnet16, out16)."""
    p16 = halves(params)
    g, _ = stage_context(p16, net16)
    z, _, rnet, _ = stage_gates(p16, g, net16, inputs16)
    z16, rnet16 = z.astype(np.float16), rnet.astype(np.float16)
    out, _ = stage_update(p16, g, z16, rnet16, net16, inputs16)
    return g, z16, rnet16, out.astype(np.float16)


# ---------------------------------------------------------------------------------------------------- packed layout
def packed_halves(hidden, c_in):
    return 9 * c_in * 3 * hidden + 4 * hidden * hidden + 7 * hidden


def _frag(w16):
    """droid_conv3x3's fragment layout of a [N,C,3,3] weight, without a bias."""
    return c3.pack(w16, np.zeros(0, dtype=np.float16))


def pack(p16):
    """[Wz; Wr] and Wq as fragments, w as [h/32][h/16][64][8] with element (s, nt, lane, j) =
    w16[16 nt + (lane & 15)][32 s + 8 (lane >> 4) + j], the context matrices row-major, then bw, bz, br, bq, bzg, brg, bqg."""
    hidden = p16["w"][0].shape[0]
    w1 = p16["w"][0].reshape(hidden, hidden)
    lane = np.arange(64)
    wf = np.empty((hidden // 32, hidden // 16, 64, 8), dtype=np.float16)
    for s in range(hidden // 32):
        for nt in range(hidden // 16):
            for j in range(8):
                wf[s, nt, :, j] = w1[16 * nt + (lane & 15), 32 * s + 8 * (lane >> 4) + j]
    parts = [_frag(np.concatenate([p16["convz"][0], p16["convr"][0]])), _frag(p16["convq"][0]), wf.reshape(-1)]
    parts += [p16[k][0].reshape(-1) for k in GLO]
    parts += [p16[k][1].reshape(-1) for k in ("w", "convz", "convr", "convq") + GLO]
    return np.concatenate(parts).astype(np.float16)


def unpack(packed, hidden, c_in):
    """The inverse of `pack`."""
    n3 = 9 * c_in * hidden
    wzr = c3.unpack(packed[:2 * n3], c_in, 2 * hidden)[0]
    wq = c3.unpack(packed[2 * n3:3 * n3], c_in, hidden)[0]
    o = 3 * n3
    hh = hidden * hidden
    wf = packed[o:o + hh].reshape(hidden // 32, hidden // 16, 4, 16, 8)          # (s, nt, g, c16, j)
    w1 = wf.transpose(1, 3, 0, 2, 4).reshape(hidden, hidden, 1, 1)                # (nt, c16, s, g, j)
    glo = [packed[o + (1 + k) * hh:o + (2 + k) * hh].reshape(hidden, hidden, 1, 1) for k in range(3)]
    b = packed[o + 4 * hh:].reshape(7, hidden)
    return {"convz": (wzr[:hidden], b[1]), "convr": (wzr[hidden:], b[2]), "convq": (wq, b[3]), "w": (np.ascontiguousarray(w1), b[0]),
            "convz_glo": (glo[0], b[4]), "convr_glo": (glo[1], b[5]), "convq_glo": (glo[2], b[6])}
