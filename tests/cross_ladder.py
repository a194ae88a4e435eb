"""The cases at which the cross frames plans (csrc/fft_plans_ext.h CrossFramesPlan: cross-spectral density, magnitude-squared
coherence, H1 transfer estimate of signal pairs on overlapping frames) are checked against float64, on the GPU
(tests/test_gpu_cross.py) and in the CPU emulation (tests/test_emulated_cross.py), with the inputs, the float64 reference and the
checks both files share.  Test infrastructure only.

A backend B runs one plan: B.run(case, kind, dt, x_ptr, x_pitch, y_ptr, y_pitch, out_ptrs, **opts) -> info executes ONE plan once
into every pointer of out_ptrs, each execute finished when it returns; info: a dict with "fused", "passes", "nw", "C", "chunks".
opts: no_fusion, and (emulation only) max_grid / block, the launch geometry of the two reduction kernels.
B.welch(case, dt, x_ptr, pitch, out_ptr): the WELCH rows of the frames plan of the same input type.

The oracle is float64 numpy: the frames are an as_strided view of the float64 / complex128 copy of each input, times the window
(frames_ladder.window_values: the reference project's formulas with their n - 1 denominators; a USER window rounded to the plan's
precision, as in the frames ladders), np.fft.rfft / fft, and
    Pxx = c_k mean_w |X_w|^2,  Pyy = c_k mean_w |Y_w|^2,  Pxy = c_k mean_w conj(X_w) Y_w,
    c_k = 1 / (fs P), doubled for 0 < k < n/2;  P = 0.375 n (Hann) or sum w^2.
The reference project's own compute_coherence is NOT an oracle: it writes 1.0 into every bin (a placeholder, "would need cross-PSD
for full implementation").

Bounds.  ALL rows, for each of Pxx, Pyy, Pxy:  error <= K u log2(n) max(RMS of the reference row over its bins, |reference bin|),
K = 8 (CROSS_K; Pxy as a complex error with |Pxy| for its RMS).  The sums run in double, so the error is that of the STFT rows (the
frames ladders' K = 8 with measured worsts <= 3.1) entering a product: about twice a row's relative error, not growing with nw.
COHERENCE and TRANSFER against the float64 values with the bound propagated to first order from those three, evaluated on the
reference: with dxx, dyy, dxy the three bounds above at a bin,
    coherence:  C (2 dxy / |Pxy| + dxx / Pxx + dyy / Pyy),      transfer:  |H| (dxy / |Pxy| + dxx / Pxx).
Every bin is checked.  The random pairs are broadband -- white noise x, y = 0.8 x[t] + 0.4 x[t-1] + 0.5 e[t] with independent
white e, so that the coherence lies between 0.39 and 0.85 and no bin of Pxy is small -- which keeps the propagated coherence bound
below 1e-2 in fp32 at every bin of every case (asserted from the float64 reference alone: test_emulated_cross.py).

Worst e / (u log2 n) measured over this ladder (profiles/cross_accuracy_report.json), fp32 / fp64:
                 Pxx            Pyy            Pxy
    MI355X       0.81 / 2.19    0.77 / 1.64    0.82 / 3.58
    emulation    0.99 / 2.19    0.84 / 1.64    0.90 / 3.58
(worst over the four paths -- real / complex input, the inner plan's one launch / fallback; per path: DESIGN.md 4.7.3.  The fp64
worsts are at n = 4 and n = 8, where log2 n leaves the unit small.)
K stays 8 only while every worst is <= 4 (tests/accuracy.py's rule: K at least twice the worst measured value).

The chunk length of the reduction is C = max(32, ceil(nw / ceil(2^18 / (S hb)))): at every shape small enough for a test C = 32
(C > 32 needs S hb nw > 2^23 frames-bins), so the chunk cases are nw = 31, 32, 33 and 75 with C read back from the plan and
asserted to be 32; the rule itself is checked as a function at large shapes (test_emulated_cross.py).
"""
import numpy as np
from numpy.lib.stride_tricks import as_strided

import accuracy as A
import frames_ladder as L
from frames_ladder import BLACKMAN, HAMMING, HANN, RECT, USER, WINDOW_NAMES  # noqa: F401

CSD, COHERENCE, TRANSFER, ALL = range(4)
KINDS = (CSD, COHERENCE, TRANSFER, ALL)
KIND_NAMES = {CSD: "csd", COHERENCE: "coherence", TRANSFER: "transfer", ALL: "all"}
CROSS_K = 8
FS = L.FS
F32, F64, C64, C128 = np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.complex64), np.dtype(np.complex128)
DTYPES = (F32, F64, C64, C128)
MIN_CHUNK = 32
TARGET_THREADS = 1 << 18


def dtype_id(dt):
    return {F32: "real-fp32", F64: "real-fp64", C64: "complex-fp32", C128: "complex-fp64"}[np.dtype(dt)]


def is_real(dt):
    return np.dtype(dt) in (F32, F64)


def real_dtype(dt):
    return F32 if np.dtype(dt) in (F32, C64) else F64


def chunk_rule(nw, n_signals, hb):
    """The plan's rule, restated: C = max(32, ceil(nw / ceil(2^18 / (S hb))))."""
    want = -(-TARGET_THREADS // (n_signals * hb))
    return max(MIN_CHUNK, -(-nw // want))


class Case(L.Case):
    """frames_ladder.Case for a pair: pad / pad_y: signal_pitch - signal_len of x and of y; dtypes: the input types the case runs;
    seed: of its random pair (one frame: the first seed at which no bin of the ONE periodogram is small enough to make the propagated
    coherence bound vacuous -- chosen on the float64 reference alone)."""

    def __init__(self, name, n, hop, n_signals, nw, tail=0, pad=0, pad_y=0, window=HANN, dtypes=DTYPES, kinds=(ALL,), seed=11, why=""):
        super().__init__(name, n, hop, n_signals, nw, tail=tail, pad=pad, window=window, kinds=kinds, dtypes=dtypes, why=why)
        self.pitch_y = self.signal_len + pad_y
        self.hb = n // 2 + 1
        self.seed = seed


REALS = (F32, F64)
SMALL = [
    Case("n4", 4, 2, 3, 5, pad=1, pad_y=2, dtypes=REALS, kinds=KINDS, why="n = 4: the real plan's fallback (a core of length 2 has no hooked kernel)"),
    Case("n8", 8, 4, 3, 7, pad=1, pad_y=3, kinds=KINDS, why="n = 8, hop = n/2, different pitches for x and y"),
    Case("n64-hop15", 64, 15, 3, 5, pad=2, pad_y=5, kinds=KINDS, why="odd hop, pitched pairs"),
    Case("n64-hop1", 64, 1, 1, 3, why="hop = 1, one pair"),
    Case("n64-hopn", 64, 64, 3, 3, why="hop = n"),
    Case("n64-tail", 64, 16, 3, 4, tail=15, why="a NaN tail no frame may read"),
    Case("n1024", 1024, 512, 1, 3, kinds=KINDS, why="n = 1024, one pair"),
    Case("one-frame", 64, 16, 3, 1, kinds=(ALL, COHERENCE), seed=12, why="nw = 1: one chunk of one frame"),
    Case("chunk-31", 8, 2, 2, 31, why="nw = C - 1: one ragged chunk"),
    Case("chunk-32", 8, 2, 2, 32, why="nw = C: one full chunk"),
    Case("chunk-33", 8, 2, 2, 33, kinds=KINDS, why="nw = C + 1: a second chunk of one frame"),
    Case("chunk-75", 8, 2, 2, 75, kinds=KINDS, why="three chunks, the last ragged"),
    Case("w-rect", 64, 16, 2, 3, window=RECT, why="window kind"),
    Case("w-hann", 64, 16, 2, 3, window=HANN, why="window kind"),
    Case("w-hamming", 64, 16, 2, 3, window=HAMMING, why="window kind"),
    Case("w-blackman", 64, 16, 2, 3, window=BLACKMAN, why="window kind"),
    Case("w-user", 64, 16, 2, 3, window=USER, kinds=KINDS, why="a random window: P = sum w^2"),
]
# one step past the real plan's one-launch range in each precision: pack, multi-pass core, split.  On the MI355X the half-length fp64
# core of 4096 still fits one hooked pass, so n = 8192 fp64 runs the one-launch path there and fp64's first fallback size is 16384
# as well: both fp64 sizes are cases.  DEVICE_FALLBACK: the cases the device must run on the inner plan's fallback.
BIG = [Case("big-fp32", 16384, 8192, 1, 3, dtypes=(F32,), why="n = 16384 fp32: the real plan's fallback, three frames"),
       Case("big-fp64", 8192, 4096, 1, 2, dtypes=(F64,), why="n = 8192 fp64: the largest one-launch frame on the device, two frames"),
       Case("big-fp64-16384", 16384, 8192, 1, 2, dtypes=(F64,), why="n = 16384 fp64: the real plan's fallback, two frames")]
DEVICE_FALLBACK = ("big-fp32", "big-fp64-16384")
IDENT = Case("ident", 64, 16, 3, 5, pad=1, pad_y=1, why="the identities: 3 pairs of 5 frames")
ONE_FRAME = next(c for c in SMALL if c.name == "one-frame")
OFFSET_CASE = Case("offset1", 64, 15, 3, 5, pad=2, pad_y=5, why="both bases one element behind a 16-byte boundary")
NO_FUSION_CASE = SMALL[2]


def user_window(case, dt):
    """The n values handed to the plan for a USER window (None otherwise), in the plan's precision."""
    return np.ascontiguousarray(L.window_values(USER, case.n).astype(real_dtype(dt))) if case.window == USER else None


def _noise(rng, shape, dt):
    if is_real(dt):
        return rng.standard_normal(shape)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def make_pair(case, dt, seed=None):
    """x [S][pitch], y [S][pitch_y] of dt: white x, y = 0.8 x[t] + 0.4 x[t-1] + 0.5 e[t]; every sample no frame covers -- the tail of
    each signal and the padding up to the pitch -- is NaN, so a frame that reads one fails its row."""
    dt = np.dtype(dt)
    rng = np.random.default_rng((case.seed if seed is None else seed, case.n, case.hop, case.n_signals, case.nw))
    S, covered = case.n_signals, (case.nw - 1) * case.hop + case.n
    xs = _noise(rng, (S, covered), dt)
    ys = 0.8 * xs + 0.4 * np.roll(xs, 1, axis=1) + 0.5 * _noise(rng, (S, covered), dt)
    nan = np.nan if is_real(dt) else np.nan + 1j * np.nan
    x = np.full((S, case.pitch), nan, dtype=dt)
    y = np.full((S, case.pitch_y), nan, dtype=dt)
    x[:, :covered] = xs
    y[:, :covered] = ys
    return x, y


def stft_rows(case, v, dt):
    """The float64 STFT rows [S][nw][hb] of one side (v: [S][its pitch])."""
    n, nw, S = case.n, case.nw, case.n_signals
    wide = np.float64 if is_real(dt) else np.complex128
    vs = np.ascontiguousarray(v.astype(wide))
    isz = vs.itemsize
    fr = as_strided(vs, shape=(S, nw, n), strides=(vs.shape[1] * isz, case.hop * isz, isz), writeable=False)
    w = window(case, dt)
    return np.fft.rfft(fr * w, axis=-1) if is_real(dt) else np.fft.fft(fr * w, axis=-1)[:, :, :case.hb]


def window(case, dt):
    return user_window(case, dt).astype(np.float64) if case.window == USER else L.window_values(case.window, case.n)


def scaling(case, dt, fs):
    """c_k, k <= n/2."""
    w = window(case, dt)
    P = 0.375 * case.n if case.window == HANN else float(np.sum(w * w))
    c = np.full(case.hb, 1.0 / (fs * P))
    c[1:case.n // 2] *= 2.0
    return c


def reference(case, x, y, dt, fs=FS):
    """(Pxx, Pyy, Pxy), each [S][hb], float64 / complex128."""
    X, Y = stft_rows(case, x, dt), stft_rows(case, y, dt)
    c = scaling(case, dt, fs)
    return c * np.mean(np.abs(X) ** 2, axis=1), c * np.mean(np.abs(Y) ** 2, axis=1), c * np.mean(np.conj(X) * Y, axis=1)


def unit(dt, n):
    return A.U[real_dtype(dt)] * max(1.0, np.log2(n))


def spectrum_bounds(case, dt, ref):
    """dxx, dyy, dxy: the absolute bound of every bin of Pxx, Pyy, Pxy, [S][hb] each."""
    out = []
    for r in ref:
        a = np.abs(r)
        rms = np.sqrt(np.mean(a ** 2, axis=-1, keepdims=True))
        out.append(CROSS_K * unit(dt, case.n) * np.maximum(rms, a))
    return out


def coherence_ref(ref):
    pxx, pyy, pxy = ref
    return np.abs(pxy) ** 2 / (pxx * pyy)


def coherence_bound(case, dt, ref):
    """C (2 dxy / |Pxy| + dxx / Pxx + dyy / Pyy) at every bin, on the reference values."""
    pxx, pyy, pxy = ref
    dxx, dyy, dxy = spectrum_bounds(case, dt, ref)
    return coherence_ref(ref) * (2.0 * dxy / np.abs(pxy) + dxx / pxx + dyy / pyy)


def transfer_bound(case, dt, ref):
    """|H| (dxy / |Pxy| + dxx / Pxx) at every bin, on the reference values."""
    pxx, pyy, pxy = ref
    dxx, dyy, dxy = spectrum_bounds(case, dt, ref)
    return np.abs(pxy / pxx) * (dxy / np.abs(pxy) + dxx / pxx)


def out_width(kind):
    """values of the real type per (pair, bin)"""
    return {CSD: 2, COHERENCE: 1, TRANSFER: 2, ALL: 4}[kind]


def decode(case, kind, raw):
    """raw [S][hb * out_width] reals -> COHERENCE: [S][hb] real; CSD / TRANSFER: [S][hb] complex; ALL: (Pxx, Pyy, Pxy)."""
    S, hb = case.n_signals, case.hb
    if kind == COHERENCE:
        return raw
    v = raw.reshape(S, hb, out_width(kind))
    if kind == ALL:
        return v[:, :, 0], v[:, :, 1], v[:, :, 2] + 1j * v[:, :, 3].astype(np.float64)
    return v[:, :, 0] + 1j * v[:, :, 1].astype(np.float64)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def execute(B, case, kind, dt, x, y=None, offset=0, label="", **opts):
    """One plan of `kind`, two executes, everything between guards.  x: [S][pitch]; y: [S][pitch_y], or None: the SAME pointer as x.
    Each input lives in a Guarded of its own, `offset` elements (a NaN each) behind its 16-byte aligned start; the outputs are
    NaN-filled between guards.  Checked: the guards of inputs and outputs; the inputs byte for byte (the NaN gaps between pitched
    signals among them); the two executes bit-identical.  Returns (raw rows [S][hb * out_width] of the real type, info)."""
    dt = np.dtype(dt)
    rdt = real_dtype(dt)
    S, width = case.n_signals, case.hb * out_width(kind)
    label = label or "%s %s %s" % (case, KIND_NAMES[kind], dtype_id(dt))
    nan = np.nan if is_real(dt) else np.nan + 1j * np.nan

    def flat(v):
        return np.concatenate([np.full(offset, nan, dtype=dt), v.reshape(-1)]).reshape(1, -1)

    fx = flat(x)
    fy = None if y is None else flat(y)
    gx = A.Guarded(1, fx.nbytes, align16=True)
    gy = None if y is None else A.Guarded(1, fy.nbytes, align16=True)
    outs = [A.Guarded(S, width * rdt.itemsize, align16=True) for _ in range(2)]
    try:
        A.upload_rows(gx, fx)
        if gy:
            A.upload_rows(gy, fy)
        for g in outs:
            g.fill(np.full(width, np.nan, dtype=rdt))
        xp = gx.ptr + offset * dt.itemsize
        yp = xp if gy is None else gy.ptr + offset * dt.itemsize
        info = B.run(case, kind, dt, xp, case.pitch, yp, case.pitch if gy is None else case.pitch_y, [g.ptr for g in outs], **opts)
        for g in outs:
            assert g.guards_intact(), "%s: the execute wrote outside its output" % label
        assert gx.guards_intact() and (gy is None or gy.guards_intact()), "%s: the execute wrote next to an input" % label
        assert A.input_unchanged(gx, fx) and (gy is None or A.input_unchanged(gy, fy)), "%s: the execute changed an input" % label
        b = A.same_bits(outs[0], outs[1], rdt, width)
        assert b is None, "%s: two executes of one plan differ at pair %d" % (label, b)
        assert info["nw"] == case.nw and info["C"] == chunk_rule(case.nw, S, case.hb) and info["chunks"] == -(-case.nw // info["C"]), (label, info)
        return outs[0].rows_at(0, S, rdt, width), info
    finally:
        for g in [gx, gy] + outs:
            if g is not None:
                g.free()


def path_name(dt, info):
    return "%s-%s" % ("real" if is_real(dt) else "complex", "fused" if info["fused"] else "fallback")


def spectrum_errors(case, dt, got, ref):
    """e, worst bin per pair for each of Pxx, Pyy, Pxy: the error of a bin in units of max(RMS of the reference row, |reference bin|)."""
    return [A.row_errors(g, r, scale="rms_or_bin") for g, r in zip(got, ref)]


def check_all(B, case, dt, x=None, y=None, offset=0, report=True, **opts):
    """The ALL rows of `case` against float64, bin by bin.  Prints each worst e / (u log2 n) before it asserts.  Returns (Pxx, Pyy, Pxy), info."""
    if x is None:
        x, y = make_pair(case, dt)
    ref = reference(case, x, y, dt)
    raw, info = execute(B, case, ALL, dt, x, y, offset=offset, **opts)
    got = decode(case, ALL, raw)
    label = "%s all %s" % (case, dtype_id(dt))
    errs = spectrum_errors(case, dt, got, ref)
    for name, (e, k) in zip(("pxx", "pyy", "pxy"), errs):
        print("%s %s: worst e / (u log2 n) = %.3f (pair %d, bin %d)" % (label, name, float(np.max(e)) / unit(dt, case.n), int(np.argmax(e)), int(k[int(np.argmax(e))])))
        if report:
            A._note("cross_%s:%s" % (name, path_name(dt, info)), real_dtype(dt), case.n, None, e)
    for name, (e, k) in zip(("pxx", "pyy", "pxy"), errs):
        A.assert_within(e, k, CROSS_K * unit(dt, case.n), "%s %s" % (label, name))
    return got, info


def _assert_bins(err, lim, label):
    bad = ~(err <= lim)
    if np.any(bad):
        s, k = np.argwhere(bad)[0]
        raise A.AccuracyError("%s: %d bins over their bound; first: pair %d bin %d, error %.3g, bound %.3g" % (label, int(np.sum(bad)), s, k, err[s, k], lim[s, k]))


def check_kind(B, case, kind, dt, x=None, y=None, **opts):
    """CSD, COHERENCE or TRANSFER rows against the float64 values, every bin within its own bound."""
    if x is None:
        x, y = make_pair(case, dt)
    ref = reference(case, x, y, dt)
    raw, info = execute(B, case, kind, dt, x, y, **opts)
    got = decode(case, kind, raw)
    label = "%s %s %s" % (case, KIND_NAMES[kind], dtype_id(dt))
    if kind == CSD:
        want, lim = ref[2], spectrum_bounds(case, dt, ref)[2]
    elif kind == COHERENCE:
        want, lim = coherence_ref(ref), coherence_bound(case, dt, ref)
    else:
        want, lim = ref[2] / ref[0], transfer_bound(case, dt, ref)
    err = np.abs(got.astype(want.dtype) - want)
    err = np.where(np.isnan(err), np.inf, err)
    print("%s: worst error / bound = %.3f" % (label, float(np.max(err / lim))))
    _assert_bins(err, lim, label)
    return got, info


def run_case(B, case, dt, **opts):
    """Every kind the case lists; returns the info of the last plan."""
    info = None
    for kind in case.kinds:
        info = (check_all(B, case, dt, **opts) if kind == ALL else check_kind(B, case, kind, dt, **opts))[1]
    return info


# ---------------------------------------------------------------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------------------------------------------------------------
def identity_same_pointer(B, dt, case=IDENT):
    """y = x through the SAME pointer: Im Pxy == 0, Pxy == Pxx == Pyy bit for bit; coherence within 4 u of 1; H1 == (1, 0)."""
    x, _ = make_pair(case, dt)
    u = A.U[real_dtype(dt)]
    raw, _ = execute(B, case, ALL, dt, x, None)
    v = raw.reshape(case.n_signals, case.hb, 4)
    assert np.all(np.isfinite(v)) and np.all(v[:, :, 0] > 0)
    assert np.all(v[:, :, 3] == 0.0), "Im Pxy of a signal with itself"
    assert bits_equal(v[:, :, 0], v[:, :, 1]) and bits_equal(v[:, :, 0], v[:, :, 2]), "Pxx, Pyy, Re Pxy of a signal with itself differ"
    coh, _ = execute(B, case, COHERENCE, dt, x, None)
    assert np.all(np.abs(coh.astype(np.float64) - 1.0) <= 4 * u), float(np.max(np.abs(coh.astype(np.float64) - 1.0))) / u
    h, _ = execute(B, case, TRANSFER, dt, x, None)
    h = h.reshape(case.n_signals, case.hb, 2)
    assert np.all(h[:, :, 0] == 1.0) and np.all(h[:, :, 1] == 0.0), "H1 of a signal with itself"


def identity_doubled(B, dt, case=IDENT):
    """y = 2 x (a buffer of its own): Pxy == 2 Pxx and Pyy == 4 Pxx bit for bit; H1 == (2, 0)."""
    x, y = make_pair(case, dt)
    covered = (case.nw - 1) * case.hop + case.n
    y[:, :covered] = 2 * x[:, :covered]
    raw, _ = execute(B, case, ALL, dt, x, y)
    v = raw.reshape(case.n_signals, case.hb, 4)
    assert np.all(np.isfinite(v)) and np.all(v[:, :, 0] > 0)
    assert bits_equal(v[:, :, 2], 2 * v[:, :, 0]) and np.all(v[:, :, 3] == 0.0), "Pxy != 2 Pxx"
    assert bits_equal(v[:, :, 1], 4 * v[:, :, 0]), "Pyy != 4 Pxx"
    h, _ = execute(B, case, TRANSFER, dt, x, y)
    h = h.reshape(case.n_signals, case.hb, 2)
    assert np.all(h[:, :, 0] == 2.0) and np.all(h[:, :, 1] == 0.0), "H1 of (x, 2x)"


def identity_swap(B, dt, case=IDENT):
    """(y, x) gives conj(Pxy) bit for bit, with Pxx and Pyy exchanged."""
    x, y = make_pair(case, dt)
    a, _ = execute(B, case, ALL, dt, x, y)
    sw = Case(case.name + "-swapped", case.n, case.hop, case.n_signals, case.nw, tail=case.tail, pad=case.pitch_y - case.signal_len,
              pad_y=case.pitch - case.signal_len, window=case.window)
    b, _ = execute(B, sw, ALL, dt, y, x)
    a, b = a.reshape(case.n_signals, case.hb, 4), b.reshape(case.n_signals, case.hb, 4)
    assert np.any(a[:, :, 3] != 0)
    assert bits_equal(a[:, :, 0], b[:, :, 1]) and bits_equal(a[:, :, 1], b[:, :, 0]), "Pxx and Pyy are not exchanged"
    # (value equality of finite numbers is bit equality but for the sign of a zero: Im Pxy of a real pair's DC and Nyquist bins is
    # +0 either way round, and its negation -0)
    assert np.all(np.isfinite(a)) and bits_equal(a[:, :, 2], b[:, :, 2]) and np.array_equal(a[:, :, 3], -b[:, :, 3]), "Pyx is not conj(Pxy) bit for bit"


def identity_one_frame(B, dt, case=ONE_FRAME):
    """nw = 1: |Pxy|^2 = Pxx Pyy, the coherence is 1 wherever both powers are nonzero.  Within 16 u: the three sums are one term
    each, formed in double -- two products and a sum, relative to |X| |Y| at most 3 * 2^-53 each even where Re or Im cancels -- then
    three scalings, two squares, a sum, a product and a quotient (about 12 * 2^-53 in all), and ONE rounding to the output type."""
    x, y = make_pair(case, dt)
    u = A.U[real_dtype(dt)]
    coh, _ = execute(B, case, COHERENCE, dt, x, y)
    ref = reference(case, x, y, dt)
    assert np.all(ref[0] > 0) and np.all(ref[1] > 0)
    d = np.abs(coh.astype(np.float64) - 1.0)
    print("one frame %s: worst |coherence - 1| = %.2f u" % (dtype_id(dt), float(np.max(d)) / u))
    assert np.all(d <= 16 * u)


def identity_welch(B, dt, case=IDENT):
    """Pxx of the cross plan against the WELCH plan on x alone: within the sum of the two bounds (this ladder's and the frames ladders')."""
    x, y = make_pair(case, dt)
    (pxx, _, _), _ = check_all(B, case, dt, x, y, report=False)
    rdt = real_dtype(dt)
    gx, gw = A.Guarded(case.n_signals, case.pitch * np.dtype(dt).itemsize, align16=True), A.Guarded(case.n_signals, case.hb * rdt.itemsize, align16=True)
    try:
        A.upload_rows(gx, x)
        B.welch(case, dt, gx.ptr, case.pitch, gw.ptr)
        w = gw.rows_at(0, case.n_signals, rdt, case.hb)
    finally:
        gx.free()
        gw.free()
    e, k = A.row_errors(pxx, w.astype(np.float64), scale="rms_or_bin")
    A.assert_within(e, k, (CROSS_K + L.BOUND_K[L.WELCH]) * unit(dt, case.n), "cross Pxx vs WELCH %s" % dtype_id(dt))


def identity_zero_x(B, dt, case=IDENT):
    """An all-zero x: Pxy, coherence and H1 exactly 0, no NaN and no Inf anywhere."""
    x, y = make_pair(case, dt)
    x = np.zeros_like(x)
    for kind in KINDS:
        raw, _ = execute(B, case, kind, dt, x, y)
        assert np.all(np.isfinite(raw)), KIND_NAMES[kind]
        if kind == ALL:
            v = raw.reshape(case.n_signals, case.hb, 4)
            assert np.all(v[:, :, 0] == 0) and np.all(v[:, :, 2] == 0) and np.all(v[:, :, 3] == 0) and np.all(v[:, :, 1] > 0)
        else:
            assert np.all(raw == 0), KIND_NAMES[kind]


def identity_poisoned_pair(B, dt, case=IDENT, pair=1):
    """A NaN / Inf in one pair (in x, then in y) leaves every other pair's rows bit-identical; a NaN pair's own rows are all NaN
    (ALL rows: but for the power of the side that was not poisoned, which stays what it was)."""
    x, y = make_pair(case, dt)
    for kind in KINDS:
        clean, _ = execute(B, case, kind, dt, x, y)
        assert np.all(np.isfinite(clean))
        for side in (0, 1):
            for poison in ("nan", "inf0"):
                px, py = (A.poisoned(x, [pair], poison), y) if side == 0 else (x, A.poisoned(y, [pair], poison))
                got, _ = execute(B, case, kind, dt, px, py)
                label = "%s %s poison=%s in %s" % (KIND_NAMES[kind], dtype_id(dt), poison, "xy"[side])
                for s in range(case.n_signals):
                    if s != pair:
                        assert bits_equal(got[s], clean[s]), "%s: pair %d changed with its neighbour" % (label, s)
                own = got[pair]
                if kind == ALL:
                    own = got[pair].reshape(case.hb, 4)
                    assert bits_equal(own[:, 1 - side], clean[pair].reshape(case.hb, 4)[:, 1 - side]), "%s: the clean side's power changed" % label
                    own = own[:, [side, 2, 3]]
                if poison == "nan":
                    assert not np.any(np.isfinite(own)), "%s: finite values in the poisoned pair's row" % label
                else:
                    assert not np.all(np.isfinite(own)), "%s: the poisoned pair's row is finite" % label


def identity_no_fusion(B, dt, case=NO_FUSION_CASE):
    """FFT_GPU_OPT_NO_FUSION: the inner plan's fallback, within the bound of float64 and within the sum of the bounds of the fused rows."""
    a, ia = check_all(B, case, dt, no_fusion=True)
    b, ib = check_all(B, case, dt)
    assert ia["fused"] == 0 and ib["fused"] == 1, (ia, ib)
    for name, g, r in zip(("pxx", "pyy", "pxy"), a, b):
        e, k = A.row_errors(g, r.astype(np.complex128 if np.iscomplexobj(r) else np.float64), scale="rms_or_bin")
        A.assert_within(e, k, 2 * CROSS_K * unit(dt, case.n), "no_fusion vs fused, %s %s" % (name, dtype_id(dt)))
