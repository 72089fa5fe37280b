"""The 27 synthetic colour videos of 24 x 40 with 4 to 8 frames (one of 12), the small ps7.yaml-format config and the
expected histories that tests/test_ps7_driver_gpu.py and tests/test_ps7_driver_shim.py share; computed once per process
from tests/_mhi_color_ref.py."""
import functools

import numpy as np

import _mhi_color_ref as R

ROWS, COLS = 24, 40
LONG = "PS7A1P1T1"  # 12 frames: the one video that reaches difference frame 10 of problem 1a
YAML = """---
input_dir: none
output_dir: none
last_frame_of_action:
{last}
mhi_action1:
  diff_threshold: 20
  pre_blur_size: 3
  pre_blur_sigma: 1
  tau: 3
  last_frame: 30
mhi_action2:
  diff_threshold: 30.5
  pre_blur_size: 3
  pre_blur_sigma: 1
  tau: 2
  last_frame: 30
mhi_action3:
  diff_threshold: 20
  pre_blur_size: {blur3}
  pre_blur_sigma: {sigma3}
  tau: 300
  last_frame: 38
...
"""


def nframes(a, p, t):
    return 12 if (a, p, t) == (1, 1, 1) else 4 + (a * 5 + p * 3 + t) % 5  # 4 .. 8


def last_frame(a, p, t):
    """F - 1 for most, earlier for some: the video runs on behind its last frame of action."""
    F = nframes(a, p, t)
    return 7 if (a, p, t) == (1, 1, 1) else (F - 1 if (p + t) % 3 else F - 2)


@functools.lru_cache(maxsize=None)
def videos():
    """A 10 x 10 block, bright in channel 0 and dark in channel 1 (differences of both signs), on texture; channel 2 is
    texture only.  Action 1: it steps by 7 columns, there and back; action 2: it hops 7 rows down and up; action 3: it
    blinks.  What a step uncovers is at least 7 x 10, enough for the open."""
    out = {}
    for a in (1, 2, 3):
        for p in (1, 2, 3):
            for t in (1, 2, 3):
                rng = np.random.default_rng(100 * a + 10 * p + t)
                F = nframes(a, p, t)
                v = rng.integers(90, 110, (F, ROWS, COLS, 3)).astype(np.uint8)
                y0, x0 = 2 + p, 2 + 2 * t
                for f in range(F):
                    if a == 1:
                        y, x = y0 + 4, x0 + 7 * (0, 1, 2, 3, 2, 1)[f % 6]
                    elif a == 2:
                        y, x = y0 + 7 * (f % 2), x0 + 10
                    elif f % 2:
                        continue
                    else:
                        y, x = y0 + 5, x0 + 12
                    assert y + 10 <= ROWS and x + 10 <= COLS
                    v[f, y:y + 10, x:x + 10, 0] = 230
                    v[f, y:y + 10, x:x + 10, 1] = 20
                v.setflags(write=False)
                out[f"PS7A{a}P{p}T{t}"] = v
    return out


def write_yaml(tmp_path, blur3=3, sigma3=1):
    lines = []
    for a in (1, 2, 3):
        lines.append(f"  action{a}:")
        for p in (1, 2, 3):
            lines.append(f"    person{p}:")
            lines += [f"      - {last_frame(a, p, t)}" for t in (1, 2, 3)]
    path = tmp_path / f"ps7_b{blur3}.yaml"
    path.write_text(YAML.format(last="\n".join(lines), blur3=blur3, sigma3=sigma3))
    return str(path)


@functools.lru_cache(maxsize=None)
def expected_mhis(blur3, sigma3):
    params = {1: (20, 3, 1, 3), 2: (30.5, 3, 1, 2), 3: (20, blur3, sigma3, 300)}
    out = []
    for a in (1, 2, 3):
        for p in (1, 2, 3):
            for t in (1, 2, 3):
                out.append(R.history_seq(videos()[f"PS7A{a}P{p}T{t}"], *params[a], (last_frame(a, p, t),))[0][0])
    return np.stack(out)
