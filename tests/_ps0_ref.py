"""The "ps0" block of include/mi_cv.h restated in numpy, from the rules stated there; it shares nothing with csrc/ or
oracle/.  CASES are shared by the GPU tests."""
import numpy as np

INT_MIN = -(1 << 31)
NAN, INF = float("nan"), float("inf")
SENTINEL = 0xA5


def cv_round(v):
    """cvRound on an array of float32 or float64: halves to even; INT_MIN for NaN, +-inf and values outside int."""
    v = np.asarray(v)
    with np.errstate(invalid="ignore"):
        r = np.rint(v.astype(np.float64))  # exact for float32 input; float64 input is rounded once, as rint does
        ok = (r >= -2147483648.0) & (r < 2147483648.0)
    return np.where(ok, np.where(ok, r, 0).astype(np.int64), INT_MIN)


def sat_u8(i):
    return np.clip(i, 0, 255).astype(np.uint8)


def mix_channels(src, m):
    src = src.reshape(src.shape[0], src.shape[1], -1)
    out = np.stack([src[:, :, k] for k in m], 2)
    return out[:, :, 0] if len(m) == 1 else out


def square(r1, c1, r2, c2, size):
    """-> (ax, ay, bx, by) or None when the square leaves an image."""
    ax, ay, bx, by = c1 // 2 - size // 2, r1 // 2 - size // 2, c2 // 2 - size // 2, r2 // 2 - size // 2
    if min(ax, ay, bx, by) < 0 or ax + size > c1 or ay + size > r1 or bx + size > c2 or by + size > r2:
        return None
    return ax, ay, bx, by


def pixel_replacement(img1, img2, size=100):
    ax, ay, bx, by = square(img1.shape[0], img1.shape[1], img2.shape[0], img2.shape[1], size)
    out = img2.copy()
    out[by:by + size, bx:bx + size] = img1[ay:ay + size, ax:ax + size]
    return out


def mean_stddev(img):
    """-> dict with the record's fields; the sums in Python integers."""
    v = img.astype(np.uint64)
    s, q, n = int(v.sum(dtype=np.uint64)), int((v * v).sum(dtype=np.uint64)), img.size
    inv = np.float64(1.0) / np.float64(n)
    mean = np.float64(s) * inv
    var = np.float64(q) * inv - mean * mean
    return {"mean": mean, "stddev": np.sqrt(max(var, np.float64(0.0))), "sum": s, "sqsum": q, "min": int(img.min()), "max": int(img.max())}


def arithmetic(img, mean, stddev):
    mean, stddev = np.float64(mean), np.float64(stddev)
    with np.errstate(all="ignore"):
        a = np.float32(np.float64(1.0) / stddev)
        t1 = sat_u8(cv_round(img.astype(np.float64) - mean))
        t2 = sat_u8(cv_round(t1.astype(np.float32) * a))
        t3 = sat_u8(cv_round(t2.astype(np.float32) * np.float32(10)))
        return sat_u8(cv_round(t3.astype(np.float64) + mean))


def subtract(a, b):
    return sat_u8(a.astype(np.int32) - b.astype(np.int32))


def translate_left2(img):
    out = np.zeros_like(img)
    out[:, :-2] = img[:, 2:]
    return out


def add_noise(img, noise):
    n = np.clip(cv_round(np.asarray(noise, np.float32)), -128, 127)
    s = np.clip(np.minimum(img.astype(np.int64), 127) + n, -128, 127)
    return np.maximum(s, 0).astype(np.uint8)


def run(image1, image2, ng, nb, size=100):
    green, red, blue = image1[:, :, 1], image1[:, :, 2], image1[:, :, 0]
    st = mean_stddev(green)
    tr = translate_left2(green)
    return {"swapped": mix_channels(image1, (2, 1, 0)), "green": green, "red": red,
            "replaced": pixel_replacement(red, image2[:, :, 2], size), "stats": st,
            "arithmetic": arithmetic(green, st["mean"], st["stddev"]), "translated": tr, "difference": subtract(green, tr),
            "noisyGreen": add_noise(green, ng), "noisyBlue": add_noise(blue, nb)}


# ---------------------------------------------------------------------------------------------------------- the cases
def image(rows, cols, ch, pad, seed):
    """(buffer with the padding at SENTINEL, the rows x cols (x ch) view of random bytes)."""
    buf = np.full((rows, cols * ch + pad), SENTINEL, np.uint8)
    view = np.ndarray((rows, cols, ch), np.uint8, buffer=buf, strides=(buf.strides[0], ch, 1))
    view[...] = np.random.default_rng(seed).integers(0, 256, (rows, cols, ch), dtype=np.uint8)
    return buf, (view[:, :, 0] if ch == 1 else view)


CHANNEL_SIZES = ((5, 7), (131, 259))
PASTE_CASES = (((100, 100), (100, 100)), ((101, 103), (101, 103)), ((131, 259), (117, 140)))
PASTE_BAD = ((99, 200), (99, 200))
ARITH_PARAMS = ((0.5, 2.0 / 3.0), (100.0, 50.0), (127.3, 0.0), (NAN, 1.0), (3.0, INF))
RUN_SIZES = (((131, 259), (117, 140)), ((100, 100), (100, 100)))
SPECIAL_NOISE = (0.5, -0.5, 1.5, -1.5, NAN, INF, -INF, 2.5, -2.5, 126.5, 127.5, -128.5, 3e9, -3e9)


def all_bytes():
    return np.arange(256, dtype=np.uint8).reshape(16, 16)


def special_noise_plane(rows, cols):
    return np.resize(np.asarray(SPECIAL_NOISE, np.float32), (rows, cols))
