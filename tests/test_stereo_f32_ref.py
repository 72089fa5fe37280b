"""The float references of disparitySSD (tests/_stereo_f32_ref.py) on the case table the GPU test runs
(tests/_stereo_float_cases.py).  No GPU.

Tied: `ssd_f32` / `ssd_serial_f32` equal the C oracle byte for byte on a thinned half of the table and on every special
kind, and equal the exact integer reference (tests/_stereo_ref.py) on 8-bit-valued pairs and -- scaled by 4 -- on dyadic
ones.  Valid: the float64 sets of `ssd_admissible` hold the order-exact answer on every finite case, and hold the two
re-associated evaluations (legal readings of the contract).  Not vacuous: on every textured (uniform, normal) pair at most 5 % of the pixels
have more than one admissible disparity, and every kernel form has a case whose answer is far from constant.  Teeth: every mutant of the contract changes the answer on cases of the path
family it aims at -- the association mutants on tile, generic and ROLLING cases separately -- and the ones that are
no legal evaluation (a window one column off, reflect-101, `<=`) fall outside the float64 sets."""
from collections import defaultdict

import numpy as np
import pytest

import _oracle as orc
import _stereo_f32_ref as R
import _stereo_float_cases as T
import _stereo_ref as iref

SPECIAL = ("halfway", "spikes", "threshold", "threshold_below", "equal", "nonfinite", "allnan")
# The mutants that have a meaning on a case, by what the case is.  (`inf_start` needs MIN_SSD_5E6.)
MUTANTS_OF = {
    "fresh sums":  ("assoc_rev", "rows_first", "wcols+1", "wcols-1", "le", "reflect101", "skip_chunk2", "inf_start"),
    "rolling":     ("assoc_rev", "fresh", "wcols+1", "wcols-1", "le", "reflect101", "skip_chunk2", "inf_start"),
    "serial":      ("half_even", "wcols+1", "wcols-1", "le", "reflect101", "skip_chunk2"),
}
COMMON = ("wcols+1", "wcols-1", "le", "reflect101")  # caught by dozens of cases each: tried on every other case only


def mutants_of(i, c):
    group = "serial" if c.flags & T.SERIAL else "rolling" if c.flags & T.ROLLING else "fresh sums"
    thinned = i % 2 == 1 and c.kind not in SPECIAL
    return [m for m in MUTANTS_OF[group]
            if not (m == "inf_start" and not c.flags & T.MIN_SSD_5E6) and not (thinned and m in COMMON)]


def reference(c, left, right, mutant=None):
    if c.flags & T.SERIAL:
        return R.ssd_serial_f32(left, right, c.rad, c.lo, c.hi, mutant=mutant)
    return R.ssd_f32(left, right, c.rad, c.lo, c.hi, c.flags, mutant=mutant)


@pytest.fixture(scope="module")
def table():
    """Per case, computed once: the pair, the reference's answer, the float64 sets (finite cuda:: path cases) and, per
    mutant, (pixels that differ from the reference, admitted everywhere?)."""
    out = {}
    for i, c in enumerate(T.CASES):
        left, right = T.make_pair(c)
        ref = reference(c, left, right)
        finite = bool(np.isfinite(left).all() and np.isfinite(right).all())
        vol = R.ssd_admissible(left, right, c.rad, c.lo, c.hi, c.flags) if finite and not c.flags & T.SERIAL else None
        muts = {}
        for m in mutants_of(i, c):
            got = reference(c, left, right, m)
            muts[m] = (int((got != ref).sum()), None if vol is None else bool(R.ssd_admits(vol, got, c.lo).all()))
        out[c.id] = (left, right, ref, vol, muts)
    return out


def test_the_table_covers_what_it_claims():
    fams = defaultdict(set)
    for c in T.CASES:
        assert c.rows <= 131 and c.cols <= 260 and -128 <= c.lo <= c.hi <= 127, c.id
        fams[c.family].add((c.rad, c.flags & ~T.MIN_SSD_5E6, c.rpw))
    for rpw in (8, 10):
        for rad in range(1, 11):
            assert {(rad, 0, rpw), (rad, T.COLS_2R, rpw)} <= fams["tile"] and (rad, T.SERIAL, rpw) in fams["serial_tile"]
    for rad in (0, 11, 15, 31):
        assert (rad, 0, 8) in fams["generic"] and (rad, T.SERIAL, 8) in fams["serial_generic"]
        assert rad == 0 or (rad, T.COLS_2R, 8) in fams["generic"]
    for rad in (0, 2, 7, 10, 11, 31):
        assert (rad, T.ROLLING, 8) in fams["rolling"] and (rad == 0 or (rad, T.ROLLING | T.COLS_2R, 8) in fams["rolling"])
    for fams_ in (("tile",), ("serial_tile",), ("generic", "serial_generic"), ("rolling",)):
        mine, fam = [c for c in T.CASES if c.family in fams_], fams_[0]
        assert {c.hi - c.lo for c in mine} >= set(T.SPANS), fam
        assert {c.pad for c in mine} == {0, 3}, fam
        assert any(c.hi < 0 for c in mine) and any(c.lo > 0 for c in mine) and any(c.lo < 0 < c.hi for c in mine), fam
    assert {c.rows for c in T.CASES if c.family == "tile"} >= set(T.ROWS)
    assert {c.rows for c in T.CASES if c.family == "serial_tile"} >= {1, 9, 31, 32, 33, 39, 40, 41}
    assert {c.rows for c in T.CASES if c.family == "rolling"} >= set(T.ROWS_ROLLING)
    assert {c.rows for c in T.CASES if c.family == "generic"} >= {1, 9, 33, 39, 40, 41}
    assert {c.rows for c in T.CASES if c.family == "serial_generic"} >= {1, 39}
    # columns: every width around the window and around a wave's 64 - 2r outputs, per family; ROLLING with an odd and an
    # even number of 64 - 2r segments (two waves per workgroup), one segment and several
    for fam in ("tile", "serial_tile"):
        seen = {w for c in T.CASES if c.family == fam
                for w, v in {"1": 1, "2r": 2 * c.rad, "2r+1": 2 * c.rad + 1, "63-2r": 63 - 2 * c.rad, "64-2r": 64 - 2 * c.rad,
                             "65-2r": 65 - 2 * c.rad, "2(64-2r)+1": 2 * (64 - 2 * c.rad) + 1}.items() if c.cols == v}
        assert seen == {"1", "2r", "2r+1", "63-2r", "64-2r", "65-2r", "2(64-2r)+1"}, (fam, seen)
    for fam in ("generic", "serial_generic"):
        assert {c.cols for c in T.CASES if c.family == fam} >= {1, 63, 64, 65, 129}, fam
        assert any(c.cols == 2 * c.rad + 1 for c in T.CASES if c.family == fam), fam
    segs = {-(-c.cols // (64 - 2 * c.rad)) for c in T.CASES if c.family == "rolling"}
    assert {1, 2, 3, 4} <= segs and any(n % 2 for n in segs if n > 4) and any(n % 2 == 0 for n in segs if n > 4), segs
    assert any(c.cols == 2 * c.rad + 1 for c in T.CASES if c.family == "rolling")
    assert {"default", "float", "host"} == {r for c in T.CASES for r in c.routes}
    assert len({c.id for c in T.CASES}) == len(T.CASES)


def test_every_form_has_a_case_that_decides_something(table):
    """A constant answer (the first disparity, or -1) is what any search returns whose cost does not depend on d.  Every
    kernel form -- family, radius, window, rows per wave -- must have a case of at least 200 pixels whose reference
    answer holds at least 6 different disparities."""
    forms = defaultdict(list)
    for c in T.CASES:
        ref = table[c.id][2]
        forms[c.family, c.rad, c.flags & T.COLS_2R, c.rpw].append((len(np.unique(ref)), ref.size, c.id))
    assert len(forms) >= 2 * 30 + 7 + 4 + 11
    for form, seen in forms.items():
        assert any(distinct >= 6 and size >= 200 for distinct, size, _ in seen), (form, seen)


def test_halfway_values_are_exactly_halfway():
    assert any(k % 2 for k in T.HALFWAY) and any(k % 2 == 0 for k in T.HALFWAY)
    for k, v in T.HALFWAY.items():
        assert v.dtype == np.float32 and np.float32(v * v) == np.float32(k + 0.5)
        assert np.floor(np.float64(np.float32(v * v)) + 0.5) == k + 1  # half away from zero


@pytest.mark.parametrize("family", T.FAMILIES)
def test_references_equal_the_oracle(table, family):
    n = 0
    for i, c in enumerate(T.CASES):
        if c.family != family or (i % 2 and c.kind not in SPECIAL):
            continue
        left, right, ref, _, _ = table[c.id]
        if c.flags & T.SERIAL:
            exp = orc.disparity_ssd_serial(left, right, c.rad, c.lo, c.hi)
        else:
            exp = orc.disparity_ssd(left, right, c.rad, c.lo, c.hi, c.flags)
        assert ref.dtype == np.int8 and np.array_equal(ref, exp), (c.id, int((ref != exp).sum()))
        n += 1
    assert n >= 3


def test_references_equal_the_integer_reference_where_sums_are_exact(table):
    """8-bit-valued pairs as they are; dyadic pairs (multiples of 1/4 in 0..8) times 4, where every cost is 16 times the
    pair's own -- without MIN_SSD_5E6, whose threshold does not scale, and not for serial::, whose rounding does not."""
    n = defaultdict(int)
    for c in T.CASES:
        left, right, ref, _, _ = table[c.id]
        if c.flags & T.ROLLING:
            continue
        if c.kind == "u8":
            if c.flags & T.SERIAL:
                exp = iref.ssd_serial(left, right, c.rad, c.lo, c.hi)
            else:
                exp = iref.ssd_cuda(left, right, c.rad, c.lo, c.hi, c.flags)
        elif c.kind == "dyadic" and not c.flags & (T.SERIAL | T.MIN_SSD_5E6):
            exp = iref.ssd_cuda(left * 4, right * 4, c.rad, c.lo, c.hi, c.flags)
        else:
            continue
        assert np.array_equal(ref, exp), (c.id, int((ref != exp).sum()))
        n[c.kind, bool(c.flags & T.SERIAL)] += 1
    assert min(n["u8", False], n["u8", True], n["dyadic", False]) >= 3, dict(n)


def test_float64_sets_hold_the_reference_and_are_mostly_singletons(table):
    shares, excluded, kept_px, all_px = {}, [], 0, 0
    for c in T.CASES:
        left, right, ref, vol, _ = table[c.id]
        if vol is None:
            continue
        ok = R.ssd_admits(vol, ref, c.lo)
        assert ok.all(), (c.id, int((~ok).sum()), np.argwhere(~ok)[:4].tolist())
        if c.kind in ("uniform", "normal"):
            # Excluded, and counted below: images no wider than the window (every candidate's window holds the whole image
            # and clamped copies of its edges), and in the others the columns where the planted match lies off the image
            # (no true minimum there: the best candidates fetch clamped edge columns, and several cost the same).
            wcols = 2 * c.rad if c.flags & T.COLS_2R else 2 * c.rad + 1
            keep = T.match_on_image(c)
            if c.cols <= wcols or not keep.any():
                excluded.append(c.id)
                continue
            kept_px += int(keep.sum()) * c.rows
            all_px += c.rows * c.cols
            shares[c.id] = float((vol.sum(0) > 1)[:, keep].mean())
    print("share of pixels with more than one admissible disparity:", {k: round(v, 4) for k, v in shares.items()})
    print(f"excluded cases ({len(excluded)}): {excluded}; pixels kept in the others: {kept_px} of {all_px}")
    textured = [c for c in T.CASES if c.kind in ("uniform", "normal") and not c.flags & T.SERIAL]
    assert len(shares) + len(excluded) == len(textured) and len(excluded) <= len(textured) // 3, (len(shares), excluded)
    assert kept_px >= 0.9 * all_px, (kept_px, all_px)
    assert {"tile", "generic", "rolling"} <= {k.split("-")[1] for k in shares}
    assert max(shares.values()) <= 0.05, {k: v for k, v in shares.items() if v > 0.05}
    # the threshold: at a cost of exactly 5e6 both -1 (the contract's answer) and a disparity are inside; just below, no -1
    for c in T.CASES:
        if c.kind in ("threshold", "threshold_below"):
            left, right, ref, vol, _ = table[c.id]
            assert (ref == (-1 if c.kind == "threshold" else c.lo)).all(), c.id
            assert vol[0].all() == (c.kind == "threshold") and vol[0].any() == (c.kind == "threshold"), c.id
        if c.kind == "equal":
            assert (table[c.id][3].sum(0) == 1).all() and (table[c.id][2] == c.lo).all(), c.id
        if c.kind == "allnan":
            assert (table[c.id][2] == -1).all(), c.id


def test_min_ssd_5e6_splits_images(table):
    """The MIN_SSD_5E6 cases are not all-found or all-rejected: per family some case holds both -1 and disparities."""
    for fam in ("tile", "generic", "rolling"):
        mixed = [c.id for c in T.CASES if c.family == fam and c.flags & T.MIN_SSD_5E6 and c.kind in ("uniform", "normal", "neartie")
                 and 0.05 < (table[c.id][2] == -1).mean() < 0.95]
        assert len(mixed) >= 1, (fam, mixed)


def test_every_mutant_is_caught_by_its_family(table):
    kills = defaultdict(lambda: defaultdict(list))  # mutant -> family -> [(case, pixels)]
    for c in T.CASES:
        for m, (n, _) in table[c.id][4].items():
            if n:
                kills[m][c.family].append((c, n))
    matrix = {m: {f: len(v) for f, v in fam.items()} for m, fam in kills.items()}
    print("cases on which each mutant differs from the reference, by family:", matrix)
    cuda = ("tile", "generic", "rolling")
    every = cuda + ("serial_tile", "serial_generic")
    want = {"assoc_rev": cuda, "rows_first": ("tile", "generic"), "wcols+1": every, "wcols-1": every, "le": every,
            "reflect101": every, "fresh": ("rolling",), "half_even": ("serial_tile", "serial_generic"), "inf_start": cuda,
            "skip_chunk2": every}
    assert set(want) == set(R.MUTANTS)
    for m, fams in want.items():
        for f in fams:
            assert kills[m][f], f"mutant {m} changes nothing on any {f} case"
    # by the kind of case that is there for it
    for f in cuda:
        for m in ("assoc_rev", "rows_first") if f != "rolling" else ("assoc_rev",):
            near = [(c.rad, n) for c, n in kills[m][f] if c.kind == "neartie" and c.rows * c.cols == 37 * 150]
            assert near and all(n >= 10 for _, n in near), (m, f, near)
            assert len(near) == sum(c.family == f and c.kind == "neartie" and c.rows * c.cols == 37 * 150 for c in T.CASES)
    assert sum(c.kind == "spikes" and n >= 10 for c, n in kills["fresh"]["rolling"]) >= 3
    for f in ("serial_tile", "serial_generic"):
        assert any(c.kind == "halfway" and n >= 10 for c, n in kills["half_even"][f]), f
    for f in every:
        assert all(c.hi - c.lo >= 64 for c, _ in kills["skip_chunk2"][f])
        assert any(c.hi - c.lo >= 65 for c, _ in kills["skip_chunk2"][f]), f
    for f in cuda:
        assert any(c.kind in ("threshold", "uniform", "normal", "neartie") for c, _ in kills["inf_start"][f]), f
    assert any(c.kind == "threshold" for c, _ in kills["inf_start"]["tile"])


def test_float64_sets_admit_legal_evaluations_and_reject_the_others(table):
    verdicts = defaultdict(lambda: [0, 0])  # mutant -> [cases admitted, cases rejected]
    for c in T.CASES:
        for m, (n, admitted) in table[c.id][4].items():
            if admitted is not None:
                verdicts[m][0 if admitted else 1] += 1
                if m in ("assoc_rev", "rows_first"):  # other associations of the same terms: inside, always
                    assert admitted, (c.id, m)
                if m == "fresh":  # fresh sums of the same terms lie inside ROLLING's (wider) intervals
                    assert admitted, (c.id, m)
    print("float64 sets, (admitted, rejected) cases per mutant:", {m: tuple(v) for m, v in verdicts.items()})
    for m in ("wcols+1", "wcols-1", "reflect101", "le", "inf_start", "skip_chunk2"):
        assert verdicts[m][1] >= 1, m
