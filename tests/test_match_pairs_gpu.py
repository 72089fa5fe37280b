"""micv_bf_match_pairs_dev (match.matchPairs): the counted matcher and the ratio test on a batch of pairs.

The contract (include/mi_cv.h): element p of idx2, dist2, match_count and the first min(match_count[p], mcap) rows of
matches_qt / distances hold the bytes of micv_bf_knn2_counted_dev(query = image pairs[p][0], train = image pairs[p][1], their
count words, caps = cap) followed by micv_bf_ratio_filter_dev over cap rows with capacity mcap.  Rows at and past that are not
written, nothing between the blocks is written, a pair index outside [0, images) is two empty lists.

References: the two single calls (byte for byte, every pair), and _ps4_feat_ref.knn2 + ratio_filter (bit for bit).  The
descriptors are 8-bit valued (test_sift_u8_gpu.planted), so every squared distance is an integer below 2^24 and exact in any
order of summation: the reference needs no tolerance.  Every output starts as a sentinel (-9 / -9.0) or as a _layout block.

dim 20 is run twice: dense (80-byte rows, a multiple of 16 bytes: the 16-byte loads) and with 84-byte rows (the scalar loads);
the _layout case takes the scalar loads as well (its planes start 4 bytes past a 256-byte boundary)."""
import numpy as np
import pytest

import _ps4_feat_ref as fr
from _layout import Plane, Slab, check as layout_check
from test_sift_u8_gpu import planted

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    from introtocomputervision_amd._capi import Context
    c = Context(0)
    yield c
    c.close()


def L():
    from introtocomputervision_amd._capi import lib
    return lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def image_set(seed, images, cap, dim=128):
    """[images, cap, dim]: planted() per image; every third row of every image is image 0's (exact matches across images, and
    with planted()'s copies exact ties), so the ratio test keeps some queries and drops others."""
    d = np.stack([planted(seed + i, cap, dim) for i in range(images)])
    d[1:, ::3] = d[0, ::3]
    return d


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_pairs(ctx, desc, counts, pairs, ratio=0.75, mcap=None, want_knn=True, pitch=None):
    """The batched call on sentinel-filled outputs -> dict of numpy arrays.  desc: [images, cap, dim] numpy or a CUDA tensor
    (any strides); counts: list / None; pairs: list or CUDA tensor."""
    from introtocomputervision_amd._capi import check
    d = desc if isinstance(desc, torch.Tensor) else dev(desc)
    images, cap, dim = d.shape
    if pitch is not None:  # rows `pitch` floats apart
        wide = torch.full((images, cap, pitch), float("nan"), device="cuda")
        wide[:, :, :dim] = d
        d = wide[:, :, :dim]
    mcap = cap if mcap is None else mcap
    pt = pairs if isinstance(pairs, torch.Tensor) else torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).cuda()
    n = pt.shape[0]
    cw = None if counts is None else torch.tensor(counts, dtype=torch.int64, device="cuda")
    o = dict(idx=torch.full((n, cap, 2), -9, dtype=torch.int32, device="cuda"),
             dist=torch.full((n, cap, 2), -9.0, device="cuda"),
             matches=torch.full((n, max(mcap, 1), 2), -9, dtype=torch.int32, device="cuda"),
             distances=torch.full((n, max(mcap, 1)), -9.0, device="cuda"),
             count=torch.full((n,), -9, dtype=torch.int64, device="cuda"))
    check(L().micv_bf_match_pairs_dev(ctx.handle, d.data_ptr(), images, d.stride(0) * 4, cap, d.stride(1) * 4,
                                      cw.data_ptr() if cw is not None else None, dim, pt.data_ptr(), n, ratio,
                                      o["idx"].data_ptr() if want_knn else None, o["dist"].data_ptr() if want_knn else None,
                                      o["matches"].data_ptr(), o["distances"].data_ptr(), mcap, o["count"].data_ptr(), stream()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def run_single(ctx, dq, dt, cq, ct, ratio=0.75, mcap=None):
    """micv_bf_knn2_counted_dev + micv_bf_ratio_filter_dev on one pair, sentinel-filled outputs."""
    from introtocomputervision_amd._capi import check
    cap, dim = dq.shape
    mcap = cap if mcap is None else mcap
    wq, wt = (torch.tensor([c], dtype=torch.int64, device="cuda") for c in (cq, ct))
    idx = torch.full((cap, 2), -9, dtype=torch.int32, device="cuda")
    dist = torch.full((cap, 2), -9.0, device="cuda")
    m = torch.full((max(mcap, 1), 2), -9, dtype=torch.int32, device="cuda")
    dd = torch.full((max(mcap, 1),), -9.0, device="cuda")
    c = torch.full((1,), -9, dtype=torch.int64, device="cuda")
    check(L().micv_bf_knn2_counted_dev(ctx.handle, dq.data_ptr(), cap, dq.stride(0) * 4, wq.data_ptr(), dt.data_ptr(), cap,
                                       dt.stride(0) * 4, wt.data_ptr(), dim, idx.data_ptr(), dist.data_ptr(), stream()))
    check(L().micv_bf_ratio_filter_dev(ctx.handle, idx.data_ptr(), dist.data_ptr(), cap, ratio, m.data_ptr(), dd.data_ptr(), mcap,
                                       c.data_ptr(), stream()))
    torch.cuda.synchronize()
    return dict(idx=idx.cpu().numpy(), dist=dist.cpu().numpy(), matches=m.cpu().numpy(), distances=dd.cpu().numpy(),
                count=int(c.item()))


def same_as_singles(ctx, desc, counts, pairs, got, mcap=None, what=""):
    d = dev(desc)
    images, cap, _ = d.shape
    memo = {}
    for p, (a, b) in enumerate(pairs):
        if (a, b) not in memo:
            ca, cb = (cap if counts is None else counts[a]), (cap if counts is None else counts[b])
            memo[a, b] = run_single(ctx, d[a], d[b], ca, cb, mcap=mcap)
        r = memo[a, b]
        w = f"{what} pair {p} = ({a}, {b})"
        assert np.array_equal(got["idx"][p], r["idx"]), w
        assert np.array_equal(got["dist"][p].view(np.uint32), r["dist"].view(np.uint32)), w
        assert got["count"][p] == r["count"], w
        n = min(r["count"], cap if mcap is None else mcap)
        assert np.array_equal(got["matches"][p][:n], r["matches"][:n]), w
        assert np.array_equal(got["distances"][p][:n].view(np.uint32), r["distances"][:n].view(np.uint32)), w
        assert (got["matches"][p][n:] == -9).all() and (got["distances"][p][n:] == -9.0).all(), f"{w}: rows past the count written"
    return memo


ALL36 = [(a, b) for a in range(6) for b in range(6)]


@pytest.mark.parametrize("counts", [(0, 1, 2, 64, 129, 300), (63, 65, 127, 128, 257, 299)])
def test_tile_edges_all_pairs(ctx, counts):
    desc = image_set(11, 6, 300)
    got = run_pairs(ctx, desc, list(counts), ALL36)
    memo = same_as_singles(ctx, desc, counts, ALL36, got, what=f"counts {counts}")
    kept = [r["count"] for r in memo.values()]
    assert max(kept) > 0 and any(0 < k < min(counts[a], 300) for (a, b), k in zip(memo, kept)), "the ratio test decided nothing"


def test_count_words_clamped_and_null(ctx):
    desc = image_set(12, 3, 70)
    pairs = [(0, 1), (1, 2), (2, 0), (1, 1), (2, 2)]
    got = run_pairs(ctx, desc, [-3, 70 + 7, 40], pairs)
    same_as_singles(ctx, desc, [-3, 70 + 7, 40], pairs, got, what="words -3, cap + 7, 40")
    clamped = run_pairs(ctx, desc, [0, 70, 40], pairs)
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), clamped[k].view(np.uint8)), k
    null = run_pairs(ctx, desc, None, pairs)
    same_as_singles(ctx, desc, None, pairs, null, what="count = NULL")
    full = run_pairs(ctx, desc, [70, 70, 70], pairs)
    for k in null:
        assert np.array_equal(null[k].view(np.uint8), full[k].view(np.uint8)), k


@pytest.mark.parametrize("dim,pitch", [(128, None), (20, None), (20, 21)])
def test_against_the_reference(ctx, dim, pitch):
    cap = 130
    desc = image_set(13 + dim, 2, cap, dim)
    counts = [cap, 97]
    pairs = [(0, 1), (1, 0), (0, 0)]
    got = run_pairs(ctx, desc, counts, pairs, pitch=pitch)
    kept = []
    for p, (a, b) in enumerate(pairs):
        nq, nt = counts[a], counts[b]
        ei, ed = fr.knn2(desc[a][:nq], desc[b][:nt])
        em, edist, ecount = fr.ratio_filter(ei, ed, 0.75)
        kept.append(ecount)
        assert np.array_equal(got["idx"][p][:nq], ei), (p, dim)
        assert np.array_equal(got["dist"][p][:nq].view(np.uint32), ed.view(np.uint32)), (p, dim)
        assert (got["idx"][p][nq:] == -1).all() and np.isposinf(got["dist"][p][nq:]).all()
        assert got["count"][p] == ecount
        assert np.array_equal(got["matches"][p][:ecount], em)
        assert np.array_equal(got["distances"][p][:ecount].view(np.uint32), edist.view(np.uint32))
    assert all(1 <= k <= cap - 1 for k in kept), f"kept {kept}: 'keep all' or 'keep none' would pass"


def test_mcap_below_the_kept_count(ctx):
    desc = image_set(14, 2, 200)
    pairs = [(0, 1), (1, 0), (1, 1)]
    full = run_pairs(ctx, desc, [200, 150], pairs)
    assert (full["count"] > 9).all()
    got = run_pairs(ctx, desc, [200, 150], pairs, mcap=9)
    same_as_singles(ctx, desc, [200, 150], pairs, got, mcap=9, what="mcap 9")
    assert np.array_equal(got["count"], full["count"]), "the count is the total kept"
    assert np.array_equal(got["matches"], full["matches"][:, :9]) and np.array_equal(got["distances"], full["distances"][:, :9])
    counts_only = run_pairs(ctx, desc, [200, 150], pairs, mcap=0)
    assert np.array_equal(counts_only["count"], full["count"])
    assert (counts_only["matches"] == -9).all() and (counts_only["distances"] == -9.0).all()


def test_containment(ctx):
    from introtocomputervision_amd._capi import check
    images, cap, dim, mcap = 3, 70, 128, 20
    desc = image_set(15, images, cap)
    counts = np.array([70, 33, 0], np.int64)
    pairs = np.array([(0, 1), (1, 0), (2, 1), (1, 2), (0, 0)], np.int32)
    n = len(pairs)
    s = Slab([Plane("desc", data=desc), Plane("count", data=counts.reshape(1, images), dense=True),
              Plane("pairs", data=pairs, dense=True),
              Plane("idx", shape=(n, cap, 2), dtype=np.int32, dense=True, tight=True),
              Plane("dist", shape=(n, cap, 2), dtype=np.float32, dense=True, tight=True),
              Plane("matches", shape=(n, mcap, 2), dtype=np.int32, dense=True, tight=True),
              Plane("distances", shape=(n, mcap, 1), dtype=np.float32, dense=True, tight=True),
              Plane("mcount", shape=(1, n), dtype=np.int64, dense=True)])
    assert s.pitch("desc") % 16 != 0 and s.dist("desc") % 16 != 0
    exp = {k: s.read(k).copy() for k in ("idx", "dist", "matches", "distances", "mcount")}  # the sentinels
    d = dev(desc)
    for p, (a, b) in enumerate(pairs):
        r = run_single(ctx, d[a], d[b], int(counts[a]), int(counts[b]), mcap=mcap)
        k = min(r["count"], mcap)
        exp["idx"][p], exp["dist"][p], exp["mcount"][0, p] = r["idx"], r["dist"], r["count"]
        exp["matches"][p][:k] = r["matches"][:k]
        exp["distances"][p][:k, 0] = r["distances"][:k]
    assert any(0 < c < mcap for c in exp["mcount"][0]) and any(c > mcap for c in exp["mcount"][0]), exp["mcount"]
    check(L().micv_bf_match_pairs_dev(ctx.handle, s.ptr("desc"), images, s.dist("desc"), cap, s.pitch("desc"), s.ptr("count"), dim,
                                      s.ptr("pairs"), n, 0.75, s.ptr("idx"), s.ptr("dist"), s.ptr("matches"), s.ptr("distances"), mcap,
                                      s.ptr("mcount"), stream()))
    torch.cuda.synchronize()
    layout_check(s, ["idx", "dist", "matches", "distances", "mcount"], exp, label="match_pairs")


def test_pair_index_out_of_range(ctx):
    desc = image_set(16, 2, 70)
    good = [(0, 1), (1, 0), (1, 1)]
    ref = run_pairs(ctx, desc, [70, 50], good)
    for bad in [(2, 0), (0, -1), (-5, 7), (0, 2 ** 31 - 1)]:
        pt = torch.tensor([good[0], bad, good[1], good[2]], dtype=torch.int32).cuda()
        got = run_pairs(ctx, desc, [70, 50], pt)
        assert (got["idx"][1] == -1).all() and np.isposinf(got["dist"][1]).all() and got["count"][1] == 0, bad
        assert (got["matches"][1] == -9).all() and (got["distances"][1] == -9.0).all(), bad
        for k in ref:
            assert np.array_equal(np.delete(got[k], 1, axis=0).view(np.uint8), ref[k].view(np.uint8)), (bad, k)


def test_pieces_and_repeat(ctx):
    """1100 pairs at cap 4096: one slice of partial lists is 1100 * 4096 * 16 bytes = 68.75 MiB, past the 64 MiB bound at any
    slicing, so the call goes in pieces; the same pairs in two calls of 550 do not."""
    images, cap = 4, 4096
    desc = np.zeros((images, cap, 128), np.float32)
    desc[:, :12] = image_set(17, images, 12)
    d = dev(desc)
    counts = [3, 10, 7, 5]
    rng = np.random.default_rng(5)
    pairs = rng.integers(0, images, (1100, 2)).astype(np.int32)
    whole = run_pairs(ctx, d, counts, dev(pairs), mcap=16)
    again = run_pairs(ctx, d, counts, dev(pairs), mcap=16)
    halves = [run_pairs(ctx, d, counts, dev(pairs[i:i + 550]), mcap=16) for i in (0, 550)]
    for k in whole:
        assert np.array_equal(whole[k].view(np.uint8), again[k].view(np.uint8)), f"{k}: a repeat differs"
        assert np.array_equal(whole[k].view(np.uint8), np.concatenate([h[k] for h in halves]).view(np.uint8)), k
    # and the halves are right: every distinct (a, b) against the single calls, on the first rows (the rest is empty)
    small = desc[:, :12]
    first = {}
    for p, (a, b) in enumerate(pairs.tolist()):
        first.setdefault((a, b), p)
    for (a, b), p in first.items():
        ei, ed = fr.knn2(small[a][:counts[a]], small[b][:counts[b]])
        em, edist, ecount = fr.ratio_filter(ei, ed, 0.75)
        assert np.array_equal(whole["idx"][p][:counts[a]], ei) and (whole["idx"][p][counts[a]:] == -1).all()
        assert whole["count"][p] == ecount and np.array_equal(whole["matches"][p][:ecount], em)


def test_existing_entries_keep_their_bytes(ctx):
    from introtocomputervision_amd import match
    q, t = dev(planted(18, 150)), dev(planted(19, 210))
    wq, wt = (torch.tensor([c], dtype=torch.int64, device="cuda") for c in (100, 133))

    def both():
        a = match.knnMatch2(q, t, ctx=ctx)
        b = match.knnMatch2Counted(q, t, wq, wt, ctx=ctx)
        return [x.cpu().numpy().view(np.uint8).copy() for x in a + b]
    before = both()
    run_pairs(ctx, image_set(20, 3, 90), [90, 1, 45], [(0, 1), (1, 2), (2, 0)])
    after = both()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    ei, ed = fr.knn2(q.cpu().numpy(), t.cpu().numpy())
    assert np.array_equal(before[0].view(np.int32), ei) and np.array_equal(before[1].view(np.uint32), ed.view(np.uint32))


def test_refusals(ctx):
    images, cap, dim, n, mcap = 2, 40, 128, 3, 40
    d = dev(image_set(21, images, cap))
    cw = torch.tensor([40, 20], dtype=torch.int64, device="cuda")
    pt = torch.tensor([(0, 1), (1, 0), (0, 0)], dtype=torch.int32).cuda()
    outs = [torch.full((n, cap, 2), -9, dtype=torch.int32, device="cuda"), torch.full((n, cap, 2), -9.0, device="cuda"),
            torch.full((n, mcap, 2), -9, dtype=torch.int32, device="cuda"), torch.full((n, mcap), -9.0, device="cuda"),
            torch.full((n,), -9, dtype=torch.int64, device="cuda")]
    good = dict(ctx=ctx.handle, desc=d.data_ptr(), images=images, dimage_stride=d.stride(0) * 4, cap=cap, dstride=d.stride(1) * 4,
                count=cw.data_ptr(), dim=dim, pairs=pt.data_ptr(), npairs=n, ratio=0.75, idx2=outs[0].data_ptr(),
                dist2=outs[1].data_ptr(), matches=outs[2].data_ptr(), distances=outs[3].data_ptr(), mcap=mcap,
                mcount=outs[4].data_ptr(), stream=stream())
    bad = [dict(ctx=None), dict(desc=None), dict(pairs=None), dict(mcount=None), dict(idx2=None), dict(dist2=None), dict(images=0),
           dict(npairs=0), dict(npairs=65536), dict(cap=0), dict(dim=0), dict(mcap=-1), dict(matches=None), dict(distances=None),
           dict(dstride=dim * 4 - 4), dict(dstride=dim * 4 + 2), dict(dstride=4 << 30), dict(dimage_stride=d.stride(0) * 4 + 2),
           dict(dimage_stride=(cap - 1) * dim * 4 + dim * 4 - 4)]
    for change in bad:
        args = dict(good, **change)
        assert L().micv_bf_match_pairs_dev(*args.values()) == EINVAL, change
        from introtocomputervision_amd._capi import last_error
        assert last_error(), change
    torch.cuda.synchronize()
    assert all(bool((o == -9).all()) for o in outs), "a refused call wrote an output"
    assert L().micv_bf_match_pairs_dev(*good.values()) == 0
    torch.cuda.synchronize()
    assert not any(bool((o == -9).all()) for o in outs)
