"""The ps7 driver of the reference (ProblemSets/ps7_cpp/src/Solution.cpp) on the device, from decoded colour frames to
confusion matrices: mhiHelper's loop with its two save sets as one call (mhi.historySequence), getAllMHIs' 27 videos as
one batch per blur (mhi.historyBatch), runProblem1's saved frames through normAndSave (display.normalizeMinMax) and
runProblem2 through the moments and the three confusion-matrix blocks.  A video is a [F, rows, cols, 3] (or
[F, rows, cols]) uint8 array of decoded frames -- a torch CUDA tensor, or a numpy array, which is uploaded once --
keyed by its file's stem, "PS7A{action}P{person}T{trial}".  Nothing here reads a result back to the host between the
calls.  matching::plotConfusionMatrix (gnuplot) is not restated."""
import numpy as np

from . import display, matching, mhi, moments

DIFF_FRAMES_1A = (10, 20, 30)  # Solution.cpp:196
PROBLEM_1B = (("PS7A1P2T1", "mhi_action1"), ("PS7A2P3T2", "mhi_action2"), ("PS7A3P2T2", "mhi_action3"))  # :208-218


def _dev(frames):
    import torch
    return frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames)).cuda()


def _reached(save, nframes):
    """An unordered_set of frame numbers as mhiHelper's loop meets them: ascending, each once, only 1 .. F - 1."""
    return sorted({int(s) for s in save if 1 <= int(s) <= nframes - 1})


def mhiHelper(frames, conf, saveDiffFrames=(), saveMHIFrames=(), ctx=None):
    """mhiHelper (Solution.cpp:16-101) over one video.  conf: config.mhi_params (diff_threshold, pre_blur_size,
    pre_blur_sigma, tau).  -> (diffFrames, mhiFrames): the {0,1} masks and the histories at the frame numbers of the two
    sets that the video reaches, in frame order, each [n, rows, cols] uint8 on the device."""
    import torch
    d = _dev(frames)
    sd, sm = _reached(saveDiffFrames, d.shape[0]), _reached(saveMHIFrames, d.shape[0])
    rows, cols = d.shape[1:3]
    if not sd and not sm:
        e = torch.empty((0, rows, cols), dtype=torch.uint8, device=d.device)
        return e, e.clone()
    out = mhi.historySequence(d, conf["diff_threshold"], conf["pre_blur_size"], conf["pre_blur_sigma"], conf["tau"], sm,
                              ctx=ctx, saveDiffFrames=sd)
    if sd:
        return out[1], out[0]
    return torch.empty((0, rows, cols), dtype=torch.uint8, device=d.device), out


def getAllMHIs(videos, cfg, ctx=None):
    """getAllMHIs (Solution.cpp:113-146): the history of every PS7A{a}P{p}T{t} (a, p, t = 1..3) at its
    last_frame_of_action, with mhi_action{a}'s parameters.  One batch call when the three actions share their blur (as
    config/ps7.yaml's do), else one per blur.  A video that is missing or ends before its last frame is left out, as
    the reference leaves it out (with an error in its log).  -> (mhis [n, rows, cols] uint8, actions [n] int32,
    people [n] int32) on the device, in the reference's order."""
    import torch
    from . import config
    last = config.last_frames(cfg)
    todo = []  # (position, frames, params, save, action, person)
    for a in (1, 2, 3):
        p = config.mhi_params(cfg, f"mhi_action{a}")
        for person in (1, 2, 3):
            for trial in (1, 2, 3):
                name = f"PS7A{a}P{person}T{trial}"
                if name in videos and name in last and 1 <= last[name] <= len(videos[name]) - 1:
                    todo.append((len(todo), _dev(videos[name]), p, last[name], a, person))
    if not todo:
        raise ValueError("getAllMHIs: no video reaches its last_frame_of_action")
    dev = todo[0][1].device
    rows, cols = todo[0][1].shape[1:3]
    out = torch.empty((len(todo), rows, cols), dtype=torch.uint8, device=dev)
    blurs = []
    for t in todo:
        b = (t[2]["pre_blur_size"], t[2]["pre_blur_sigma"])
        if b not in blurs:
            blurs.append(b)
    for b in blurs:
        grp = [t for t in todo if (t[2]["pre_blur_size"], t[2]["pre_blur_sigma"]) == b]
        res = mhi.historyBatch([t[1] for t in grp], [t[2]["diff_threshold"] for t in grp], b[0], b[1],
                               [t[2]["tau"] for t in grp], [t[3] for t in grp], ctx=ctx)
        if len(blurs) == 1:
            out = res
        else:
            out[torch.tensor([t[0] for t in grp], device=dev)] = res
    return (out, torch.tensor([t[4] for t in todo], dtype=torch.int32, device=dev),
            torch.tensor([t[5] for t in todo], dtype=torch.int32, device=dev))


def runProblem1(videos, cfg, ctx=None):
    """sol::runProblem1 (:188-223) -> {"ps7-1-a-1" .. "-3": difference frames 10, 20, 30 of PS7A1P1T1 (those the video
    reaches), "ps7-1-b-1" .. "-3": the histories of PS7A1P2T1, PS7A2P3T2, PS7A3P2T2 at their last frames}, each through
    normAndSave's cv::normalize(0, 255, NORM_MINMAX): [rows, cols] uint8 on the device."""
    from . import config
    last = config.last_frames(cfg)
    out = {}
    diffs, _ = mhiHelper(videos["PS7A1P1T1"], config.mhi_params(cfg, "mhi_action1"), DIFF_FRAMES_1A, (), ctx=ctx)
    if diffs.shape[0]:
        for i, img in enumerate(display.normalizeMinMax(diffs, ctx=ctx)):
            out[f"ps7-1-a-{i + 1}"] = img
    for i, (name, section) in enumerate(PROBLEM_1B):
        _, hist = mhiHelper(videos[name], config.mhi_params(cfg, section), (), (last[name],), ctx=ctx)
        if not hist.shape[0]:
            raise ValueError(f"runProblem1: {name} ends before its last_frame_of_action {last[name]}")
        out[f"ps7-1-b-{i + 1}"] = display.normalizeMinMax(hist[0], ctx=ctx)
    return out


def runProblem2(videos, cfg, ctx=None):
    """sol::runProblem2 (:225-318) without the plots: getAllMHIs, energyFromHistory, the moments of the NORM_INF
    histories and of the energies, naiveConfusionMatrix on mu and on eta, confusionMatrix on mu per person.  -> a dict
    of device tensors: "mhis", "meis" [n, rows, cols]; "actions", "people"; "mhi_mu", "mhi_eta", "mei_mu", "mei_eta"
    [n, 7]; "ps7-2-a-1", "ps7-2-a-2" [3, 3]; "ps7-2-b" [4, 3, 3] (persons 1..3, then the average)."""
    mhis, actions, people = getAllMHIs(videos, cfg, ctx=ctx)
    n, rows, cols = mhis.shape
    meis = mhi.energyFromHistory(mhis.view(n * rows, cols), ctx=ctx).view(n, rows, cols)  # (one launch over the stack)
    mu, eta, _ = moments.centralMomentsBatch(mhis, normInf=True, ctx=ctx)
    emu, eeta, _ = moments.centralMomentsBatch(meis, ctx=ctx)
    return {"mhis": mhis, "meis": meis, "actions": actions, "people": people, "mhi_mu": mu, "mhi_eta": eta,
            "mei_mu": emu, "mei_eta": eeta,
            "ps7-2-a-1": matching.naiveConfusionMatrix(mu, actions, ctx=ctx)[0],
            "ps7-2-a-2": matching.naiveConfusionMatrix(eta, actions, ctx=ctx)[0],
            "ps7-2-b": matching.confusionMatrix(mu, actions, people, 3, ctx=ctx)[0]}
