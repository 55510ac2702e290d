"""The contract of droid_ba_inputs (include/droid_update_hip.h) restated in numpy, edge by edge and frame by frame, and
the table of cases the CPU and the GPU tests share.  tests/test_ba_inputs_ref.py holds this restatement against the stock
tail of FactorGraph.update written with torch operators on the CPU."""
import numpy as np

F16, F32 = np.float16, np.float32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
TILE_PIXELS = 1024                       # pixels one workgroup of the streaming launch covers (256 threads x 4)
SENTINEL_F32 = 0x7FC0DEAD                # a NaN pattern nothing here computes
SENTINEL_I64 = -0x0123456789ABCDEF
SENTINEL_I32 = 0x5EADBEEF


class Case:
    """The arguments of one call as numpy arrays (None where the contract allows NULL)."""

    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name


def _sat(v):
    return int(min(max(int(v), INT_MIN), INT_MAX))


def reference(c):
    """Every output of the call on case c, as a dict; damping_buf is the buffer after the call."""
    ii, jj, nbuf = c.ii, c.jj, c.nbuf
    E, Ei = len(ii), len(c.ii_inac)
    h, w = c.a.shape[1:3]
    t0 = int(c.t0) if c.t0 >= 0 else max(1, min(int(v) for v in ii) + 1)
    kept = [k for k in range(Ei) if int(c.ii_inac[k]) >= t0 - 3 and int(c.jj_inac[k]) >= t0 - 3]
    K, Eb = len(kept), len(kept) + E
    ii_ba = np.array([c.ii_inac[k] for k in kept] + list(ii), np.int64)
    jj_ba = np.array([c.jj_inac[k] for k in kept] + list(jj), np.int64)
    inside = lambda v: 0 <= int(v) < nbuf   # noqa: E731
    A = sorted({int(v) for v in ii if inside(v)})
    U = sorted({int(v) for v in ii_ba if inside(v)})
    flags = 0
    if not all(inside(v) for v in ii_ba) or not all(inside(v) for v in jj_ba):
        flags |= 1
    n_damp = 0 if c.damping_net is None else len(c.damping_net)
    if c.damping_net is not None and n_damp != len(A):
        flags |= 2
    t1 = max(max(int(v) for v in ii_ba), max(int(v) for v in jj_ba)) + 1

    # per active edge, fp32: one addition, exact widening
    if c.delta is not None:
        target = c.a + c.delta.astype(F32)
        weight = c.w.astype(F32)
        state = (target.copy(), weight.copy())
    else:
        target, weight = c.a, c.w
        assert weight.dtype == F32
        state = (None, None)
    target_ba = np.empty((Eb, 2, h, w), F32)
    weight_ba = np.empty((Eb, 2, h, w), F32)
    for r in range(Eb):
        t, wt = (c.target_inac[kept[r]], c.weight_inac[kept[r]]) if r < K else (target[r - K], weight[r - K])
        for comp in (0, 1):
            target_ba[r, comp] = t[:, :, comp]
            weight_ba[r, comp] = wt[:, :, comp]

    buf = c.damping_buf.copy()
    for g, f in enumerate(A):
        if g < n_damp:
            buf[f] = c.damping_net[g].astype(F32)
    eta = np.empty((len(U), h, w), F32)
    for i, f in enumerate(U):
        prod = (F32(0.2) * buf[f]).astype(F32)          # rounded before the addition: two roundings
        eta[i] = (prod + F32(c.ep)).astype(F32)
    return dict(Eb=Eb, M=len(U), G=len(A), K=K, t0=_sat(t0), t1=_sat(t1), flags=flags, ii_ba=ii_ba, jj_ba=jj_ba,
                target_ba=target_ba, weight_ba=weight_ba, target_state=state[0], weight_state=state[1], eta=eta,
                frames_active=np.array(A, np.int64), frames_eta=np.array(U, np.int64), damping_buf=buf)


def info_of(ref):
    return np.array([ref["Eb"], ref["M"], ref["G"], ref["t0"], ref["t1"], ref["flags"], ref["K"], 0], np.int32)


def same_bits(a, b):
    """Bit for bit, except that any NaN matches any NaN (the payload is not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    bits = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(bits)[~na], b.view(bits)[~nb]))


# ------------------------------------------------------------------------------------------------------------ the cases
def _special(x, kind):
    """IEEE specials at fixed places of a network output, as far as it has room for them"""
    flat = x.reshape(-1)
    if kind == "delta":
        vals = [np.nan, np.inf, -np.inf, -0.0, 65504.0, -65504.0, 5.96e-8, -5.96e-8, 6.0e-5 / 3]   # half subnormals too
    else:
        vals = [0.0, 1.0, 0.0, 1.0]
    for k, v in enumerate(vals):
        if 3 * k + 1 < flat.size:
            flat[3 * k + 1] = v


def make(name, h, w, ii, jj, ii_inac=(), jj_inac=(), nbuf=16, t0=-1, net=F16, damp=F16, n_damp=None, damping=True,
         emit_only=False, ep=1e-7, special=False, zero_damping_row=None, seed=0):
    rng = np.random.default_rng(seed + 1000 * h + w)
    ii, jj = np.array(ii, np.int64), np.array(jj, np.int64)
    ii_inac, jj_inac = np.array(ii_inac, np.int64), np.array(jj_inac, np.int64)
    E, Ei = len(ii), len(ii_inac)
    a = rng.uniform(-3, 70, (E, h, w, 2)).astype(F32)
    delta = w_net = None
    if emit_only:
        w_net = rng.uniform(0, 1, (E, h, w, 2)).astype(F32)
    else:
        delta = rng.normal(0, 2, (E, h, w, 2)).astype(net)
        w_net = rng.uniform(0, 1, (E, h, w, 2)).astype(net)
        if special:
            _special(delta, "delta")
            a.reshape(-1)[-1:] = -0.0
            delta.reshape(-1)[-1:] = 0.0       # -0.0 + 0.0
    _special(w_net, "weight")
    G = len({int(v) for v in ii if 0 <= v < nbuf})
    damping_net = None
    if damping and not emit_only:
        rows = G if n_damp is None else n_damp
        damping_net = rng.uniform(1e-3, 1, (rows, h, w)).astype(damp)
        if zero_damping_row is not None:
            damping_net[zero_damping_row] = 0         # eta == ep exactly
    buf = rng.uniform(1e-3, 1, (nbuf, h, w)).astype(F32)
    return Case(name, h=h, wd=w, nbuf=nbuf, t0=t0, ep=ep, ii=ii, jj=jj, a=a, delta=delta, w=w_net,
                damping_net=damping_net, damping_buf=buf, ii_inac=ii_inac, jj_inac=jj_inac,
                target_inac=rng.uniform(-3, 70, (Ei, h, w, 2)).astype(F32),
                weight_inac=rng.uniform(0, 1, (Ei, h, w, 2)).astype(F32))


def _big():
    rng = np.random.default_rng(77)
    frames = np.sort(rng.choice(np.arange(40, 512), 300, replace=False))   # sources over 15 bitmap words
    ii = frames[rng.integers(0, 300, 2500)]
    ii[:300] = frames
    jj = rng.integers(0, 512, 2500)
    ii_inac = rng.integers(0, 512, 1300)      # some below t0' - 3 = 38 (dropped), some sources of their own
    jj_inac = rng.integers(20, 512, 1300)
    return make("big_2500_edges", 1, 2, ii, jj, ii_inac, jj_inac, nbuf=512, seed=5)


def cases():
    big = 2 ** 40
    out = [
        make("no_inactive_5x7", 5, 7, [3, 4, 4, 5, 6, 6, 7], [4, 3, 5, 4, 7, 5, 6], nbuf=9, seed=1),
        # t0' = 8: the threshold is 5, by ii and by jj
        make("boundary_6x9", 6, 9, [7, 8, 8, 9, 10, 11], [8, 7, 9, 8, 11, 10], [5, 4, 9, 9, 5, 4], [9, 9, 5, 4, 5, 4],
             nbuf=12, seed=2),
        make("all_kept_8x16", 8, 16, [12, 13, 14, 15, 15], [13, 12, 15, 14, 12],
             [10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15], [11, 12, 10, 12, 10, 11, 15, 14, 10, 11, 10, 11], nbuf=20, seed=3),
        make("all_dropped_16x16_f32", 16, 16, list(range(20, 40)), list(range(21, 40)) + [20], [1, 2, 3, 16], [2, 3, 4, 30],
             nbuf=40, net=F32, damp=F32, seed=4),
        make("t0_none_min_0_1x1", 1, 1, [0, 1, 2], [1, 0, 1], [0, 1], [2, 2], nbuf=9, seed=5),
        make("explicit_t0_5x7", 5, 7, [6, 7, 8], [7, 6, 7], [1, 2, 3, 4, 5], [2, 1, 2, 5, 4], nbuf=10, t0=5, seed=6),
        # 6 and 7 repeat, 6 is active and inactive, 4 is a source of inactive edges only
        make("shared_and_inactive_only_sources_6x9", 6, 9, [6, 6, 7, 7, 8], [7, 8, 6, 8, 6], [6, 4, 4], [4, 6, 7], nbuf=11,
             t0=3, seed=7),
        make("frames_0_and_last_8x16", 8, 16, [0, 14, 14, 7], [14, 0, 7, 0], [14], [1], nbuf=15, seed=8),
        make("outside_explicit_t0_5x7", 5, 7, [3, -1, 4], [9, 2, big], [big, 2], [3, 3], nbuf=9, t0=2, seed=9),
        make("outside_min_ii_6x9", 6, 9, [3, -1, 4], [2, 2, 3], [1], [-1], nbuf=9, seed=10),
        make("n_damp_below_G_5x7", 5, 7, [2, 3, 4, 5], [3, 2, 5, 4], nbuf=9, n_damp=2, seed=11),
        make("n_damp_above_G_5x7", 5, 7, [2, 3, 4, 5], [3, 2, 5, 4], [1], [2], nbuf=9, n_damp=6, seed=12),
        make("no_damping_8x16", 8, 16, [2, 3, 3], [3, 2, 4], [2], [3], nbuf=9, damping=False, seed=13),
        make("emit_only_6x9", 6, 9, [2, 3, 3, 9], [3, 2, 4, 8], nbuf=12, emit_only=True, seed=14),
        make("emit_only_inactive_5x7", 5, 7, [4, 5, 5], [5, 4, 6], [2, 0], [3, 4], nbuf=9, emit_only=True, seed=15),
        make("specials_half_5x7", 5, 7, [2, 3, 4], [3, 2, 3], [1], [2], nbuf=9, special=True, zero_damping_row=1, seed=16),
        make("specials_f32_8x16", 8, 16, [2, 3, 4], [3, 2, 3], [1], [2], nbuf=9, net=F32, damp=F32, special=True,
             zero_damping_row=0, seed=17),
        make("half_net_f32_damping_6x9", 6, 9, [2, 3], [3, 2], nbuf=9, damp=F32, seed=18),
        make("f32_net_half_damping_16x16", 16, 16, [2, 3], [3, 2], [2], [3], nbuf=9, net=F32, seed=19),
        make("tile_plus_one_25x41", 25, 41, [2, 3], [3, 2], [1], [2], nbuf=9, seed=20),
        _big(),
    ]
    assert any(c.h * c.wd == TILE_PIXELS + 1 for c in out)
    return out


CASES = cases()
