"""Exact numpy restatement of ps6's ParticleFilter (ProblemSets/ps6_cpp/lib/ParticleFilter.cpp) with the decisions
include/mi_cv.h ("ps6: particle filter") and DESIGN.md section 2 record: cv::RNG and its ziggurat, the fresh-generator
quirk, the saturating u8 MSE, the histogram chi-square, the library's own exp, the weights, the clamped resampling,
the sequential float estimate and the model update.  Imports no library code.

`PF(...)` mirrors micv_pf_create; `tick(frame)` returns (x, y, x_var, y_var, status).  The keyword `mutate` switches
one contract decision to a plausible alternative (the tests check each one changes a result):
  "rng_continues"   one generator carried across ticks for the displacements and the resampling uniforms
  "mse_unsaturated" (m - c)^2 with the flag off
  "unclamped"       an upper_bound past the end wraps to particle 0 instead of clamping to n - 1
  "float_simsum"    simSum accumulated in float
  "fused_blend"     the model blend as one fused multiply-add
"""
import math

import numpy as np

F32 = np.float32
RNG_FLT = F32(2.3283064365386962890625e-10)
FLT_MIN = F32(1.17549435082228750797e-38)
DBL_EPSILON = 2.220446049250313e-16
MSE, HIST = 0, 1
MSE_SIGNED = 1
STATUS_NO_WEIGHT, STATUS_CLAMPED = 1, 2
BINS = 32

# ------------------------------------------------------------------------------------------- exp


def pf_exp(x):
    """The library's double exp: fdlibm's reduction and rational form, evaluated step by step."""
    x = float(x)
    if x != x:
        return x
    if x > 7.09782712893383973096e+02:
        return math.inf
    if x < -7.45133219101941108420e+02:
        return 0.0
    k = int(x * 1.44269504088896338700e+00 + (-0.5 if x < 0 else 0.5))
    hi = x - float(k) * 6.93147180369123816490e-01
    lo = float(k) * 1.90821492927058770002e-10
    r = hi - lo
    t = r * r
    c = r - t * (1.66666666666666019037e-01 + t * (-2.77777777770155933842e-03 + t * (
        6.61375632143793436117e-05 + t * (-1.65339022054652515390e-06 + t * 4.13813679705723846039e-08))))
    y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
    if k > 1000:
        return (y * math.ldexp(1.0, 1000)) * math.ldexp(1.0, k - 1000)
    if k < -1000:
        return (y * math.ldexp(1.0, k + 1000)) * math.ldexp(1.0, -1000)
    return y * math.ldexp(1.0, k)


# ------------------------------------------------------------------------------------------- cv::RNG


def _tables():
    m1 = 2147483648.0
    dn = tn = 3.442619855899
    vn = 9.91256303526217e-3
    kn = [0] * 128
    wn = [F32(0)] * 128
    fn = [F32(0)] * 128
    q = vn / pf_exp(-.5 * dn * dn)
    kn[0] = int((dn / q) * m1)
    kn[1] = 0
    wn[0] = F32(q / m1)
    wn[127] = F32(dn / m1)
    fn[0] = F32(1.0)
    fn[127] = F32(pf_exp(-.5 * dn * dn))
    for i in range(126, 0, -1):
        dn = math.sqrt(-2. * math.log(vn / dn + pf_exp(-.5 * dn * dn)))
        kn[i + 1] = int((dn / tn) * m1)
        tn = dn
        fn[i] = F32(pf_exp(-.5 * dn * dn))
        wn[i] = F32(dn / m1)
    return kn, wn, fn


KN, WN, FN = _tables()


def _logf(v):
    return F32(math.log(float(v)))


class CvRng:
    """cv::RNG: multiply-with-carry, state 0xffffffff by default (and for a seed of 0)."""

    def __init__(self, seed=0xFFFFFFFF):
        self.state = seed if seed else 0xFFFFFFFF

    def _step(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF

    def next(self):
        self._step()
        return self.state & 0xFFFFFFFF

    def uniform(self, a, b):
        a, b = F32(a), F32(b)
        u = F32(F32(self.next()) * RNG_FLT)
        return F32(F32(u * F32(b - a)) + a)

    def gaussian(self, sigma):
        """randn_0_1_32f (a word is read BEFORE the state steps) times sigma in double."""
        while True:
            w = self.state & 0xFFFFFFFF
            hz = w - (1 << 32) if w >= 1 << 31 else w
            self._step()
            iz = hz & 127
            x = F32(F32(hz) * WN[iz])
            if abs(hz) < KN[iz]:  # (abs(INT_MIN) as unsigned is 2^31: never below a table entry)
                break
            if iz == 0:
                while True:
                    x = F32(F32(self.state & 0xFFFFFFFF) * RNG_FLT)
                    self._step()
                    y = F32(F32(self.state & 0xFFFFFFFF) * RNG_FLT)
                    self._step()
                    x = F32(float(-_logf(F32(x + FLT_MIN))) * 0.2904764)
                    y = F32(-_logf(F32(y + FLT_MIN)))
                    if not (F32(y + y) < F32(x * x)):
                        break
                x = F32(F32(3.442620) + x) if hz > 0 else F32(F32(-F32(3.442620)) - x)
                break
            y = F32(F32(self.state & 0xFFFFFFFF) * RNG_FLT)
            self._step()
            lhs = F32(FN[iz] + F32(y * F32(FN[iz - 1] - FN[iz])))
            if float(lhs) < pf_exp(-.5 * float(x) * float(x)):
                break
        return float(x) * float(sigma)


def displacement_table(seed, n, sigma):
    rng = CvRng(seed)
    out = np.empty((n, 2), np.float64)
    for i in range(n):
        out[i, 0] = rng.gaussian(sigma)
        out[i, 1] = rng.gaussian(sigma)
    return out


def uniform_table(seed, n):
    rng = CvRng(seed)
    return np.array([rng.uniform(0.0, 1.0) for _ in range(n)], np.float32)


def gen_particles(seed, n, uniform, xmax, ymax, sigma, cx, cy, max_tries=None):
    """genParticles: exact duplicates (float ==) drawn again; None when n distinct pairs do not come."""
    rng = CvRng(seed)
    seen = set()
    out = []
    tries = 64 * n + 4096 if max_tries is None else max_tries
    for _ in range(tries):
        if len(out) == n:
            break
        if uniform:
            x = rng.uniform(0.0, xmax)
            y = rng.uniform(0.0, ymax)
        else:
            x = F32(rng.gaussian(sigma) + float(cx))
            y = F32(rng.gaussian(sigma) + float(cy))
        key = (float(x), float(y))
        if key not in seen:
            seen.add(key)
            out.append(key)
    return np.array(out, np.float32).reshape(-1, 2) if len(out) == n else None


# ------------------------------------------------------------------------------------------- scoring


def patch_at(frame, x0, y0, mrows, mcols):
    """The mrows x mcols patch whose top-left frame pixel is (x0, y0), BORDER_REPLICATE outside."""
    f = frame if frame.ndim == 3 else frame[:, :, None]
    ri = np.clip(np.arange(mrows) + y0, 0, f.shape[0] - 1)
    ci = np.clip(np.arange(mcols) + x0, 0, f.shape[1] - 1)
    return f[ri][:, ci]


def cv_round(v):
    return int(np.rint(F32(v)))


def mse_sum(model, cand, signed, unsaturated=False):
    d = model.astype(np.int64) - cand.astype(np.int64)
    if signed or unsaturated:
        return int((d * d).sum())
    return int(np.minimum(np.maximum(d, 0) ** 2, 255).sum())


def norm_hist(patch):
    """Per channel: 32 bins of v >> 3, cv::normalize(NORM_L2) as h * (1 / sqrt(sum h^2)) in double -> float."""
    p = patch.reshape(-1, patch.shape[-1])
    out = np.empty((p.shape[1], BINS), np.float32)
    for c in range(p.shape[1]):
        h = np.bincount(p[:, c] >> 3, minlength=BINS).astype(np.int64)
        inv = 1.0 / math.sqrt(float(int((h * h).sum())))
        out[c] = (h.astype(np.float64) * inv).astype(np.float32)
    return out


def chi_square(a, b):
    """HISTCMP_CHISQR: sum in bin order of d^2 / a over |a| > DBL_EPSILON, d = a - b in float."""
    s = 0.0
    for j in range(len(a)):
        if abs(float(a[j])) > DBL_EPSILON:
            d = float(F32(a[j] - b[j]))
            s += d * d / float(a[j])
    return s


def seq_sum_f32(v):
    v = np.asarray(v, np.float32)
    return F32(0) if len(v) == 0 else np.add.accumulate(v, dtype=np.float32)[-1]


def seq_sum_f64(v):
    s = 0.0
    for x in np.asarray(v, np.float64):
        s += float(x)
    return s


class PF:
    def __init__(self, model, img_rows, img_cols, n, mode, mse_sigma, sample_sigma, init=(-1.0, -1.0), alpha=0.1,
                 flags=0, seed=0xFFFFFFFF, mutate=None):
        model = np.asarray(model, np.uint8)
        self.model0 = model if model.ndim == 3 else model[:, :, None]
        self.model0 = np.ascontiguousarray(self.model0)
        self.mrows, self.mcols, self.ch = self.model0.shape
        self.rows, self.cols, self.n, self.mode = img_rows, img_cols, n, mode
        self.mse_sigma, self.flags, self.mutate = float(mse_sigma), flags, mutate
        self.fa, self.fb = F32(alpha), F32(1.0 - float(alpha))
        self.model = self.model0.copy()
        self.hist = norm_hist(self.model0) if mode == HIST else np.zeros((self.ch, BINS), np.float32)
        ix, iy = F32(init[0]), F32(init[1])
        uniform = ix == F32(-1) and iy == F32(-1)
        cx = F32(ix + F32(F32(self.mcols) / F32(2)))
        cy = F32(iy + F32(F32(self.mrows) / F32(2)))
        self.particles = gen_particles(seed, n, uniform, F32(img_cols), F32(img_rows), sample_sigma, cx, cy)
        if self.particles is None:
            raise ValueError("cannot draw n distinct particles")
        self.weights = np.full(n, F32(1) / F32(n), np.float32)
        self.seed, self.sample_sigma = seed, sample_sigma
        self.disp = displacement_table(seed, n, sample_sigma)
        self.uni = uniform_table(seed, n)
        self._rng = CvRng(seed)  # the "rng_continues" mutation's one generator

    def _tables(self):
        if self.mutate != "rng_continues":
            return self.disp, self.uni
        d = np.array([[self._rng.gaussian(self.sample_sigma), self._rng.gaussian(self.sample_sigma)]
                      for _ in range(self.n)], np.float64)
        return d, np.array([self._rng.uniform(0.0, 1.0) for _ in range(self.n)], np.float32)

    def similarity(self, frame, px, py):
        x0 = cv_round(px) - (self.mcols + 1) // 2
        y0 = cv_round(py) - (self.mrows + 1) // 2
        cand = patch_at(frame, x0, y0, self.mrows, self.mcols)
        if self.mode == MSE:
            s = mse_sum(self.model, cand, self.flags & MSE_SIGNED, self.mutate == "mse_unsaturated")
            mse = s / float(self.mrows * self.mcols)
            return pf_exp(-mse / (2 * self.mse_sigma * self.mse_sigma))
        h = norm_hist(cand)
        comp = 0.0
        for c in range(self.ch):
            comp += chi_square(self.hist[c], h[c])
        comp /= float(self.ch)
        return pf_exp(-comp)

    def tick(self, frame):
        frame = np.asarray(frame, np.uint8)
        disp, uni = self._tables()
        n = self.n
        moved = np.empty((n, 2), np.float32)
        moved[:, 0] = (self.particles[:, 0].astype(np.float64) + disp[:, 0]).astype(np.float32)
        moved[:, 1] = (self.particles[:, 1].astype(np.float64) + disp[:, 1]).astype(np.float32)
        sims = np.zeros(n, np.float64)
        for i in range(n):
            px, py = moved[i]
            if px >= 0 and px < F32(self.cols) and py >= 0 and py < F32(self.rows):
                sims[i] = self.similarity(frame, px, py)
        w0 = sims.astype(np.float32)
        if self.mutate == "float_simsum":
            simsum = float(seq_sum_f32(w0))
        else:
            simsum = seq_sum_f64(sims)
        status = 0
        if simsum == 0.0 or not math.isfinite(simsum):
            status |= STATUS_NO_WEIGHT
            self.weights = w0
            idx = np.arange(n)
        else:
            self.weights = (w0.astype(np.float64) / simsum).astype(np.float32)
            cum = np.add.accumulate(self.weights, dtype=np.float32)
            idx = np.searchsorted(cum, uni, side="right")  # std::upper_bound (cum is non-decreasing)
            if (idx >= n).any():
                status |= STATUS_CLAMPED
            idx = np.where(idx >= n, 0 if self.mutate == "unclamped" else n - 1, idx)
        self.particles = moved[idx]
        xm = F32(seq_sum_f32(self.particles[:, 0]) / F32(n))
        ym = F32(seq_sum_f32(self.particles[:, 1]) / F32(n))
        dx = self.particles[:, 0] - xm
        dy = self.particles[:, 1] - ym
        xv = F32(seq_sum_f32(dx * dx) / F32(n))
        yv = F32(seq_sum_f32(dy * dy) / F32(n))
        self._update_model(frame, xm, ym)
        return (xm, ym, xv, yv, status)

    def _update_model(self, frame, xm, ym):
        lim = F32(16777216.0)
        ex = min(max(F32(xm), -lim), lim)
        ey = min(max(F32(ym), -lim), lim)
        new = patch_at(frame, cv_round(ex) - (self.mcols + 1) // 2, cv_round(ey) - (self.mrows + 1) // 2,
                       self.mrows, self.mcols)
        old = self.model0 if self.mode == HIST else self.model
        if self.mutate == "fused_blend":
            t = (new.astype(np.float64) * float(self.fa) + (old.astype(np.float32) * self.fb).astype(np.float64))
            t = t.astype(np.float32)
        else:
            t = new.astype(np.float32) * self.fa + old.astype(np.float32) * self.fb
        self.model = np.clip(np.rint(t), 0, 255).astype(np.uint8)
        if self.mode == HIST:
            self.hist = norm_hist(self.model)
