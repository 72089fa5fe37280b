#!/usr/bin/env python3
"""Compiler resource report of the Harris image -> R kernels, and the proof that the byte source left the f32
instantiations alone.

    python tools/harris_u8_resources.py [--parent PARENT_harris.hip] > profiles/harris_u8/resources.txt

Compiles csrc/harris.hip and csrc/harris_u8.hip for gfx950 (device side only; no GPU needed), prints VGPRs, SGPRs, scratch,
LDS and occupancy of every harris_image_response[_u8]_kernel instantiation and of the list / keypoint kernels, and -- when
the parent commit's harris.hip is given -- compares the instruction streams of the f32 instantiations with the parent's,
line by line (labels and comments dropped)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "introtocomputervision_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-fno-gpu-flush-denormals-to-zero", "-Wall", "-Wno-unused-function", "--cuda-device-only", "-S",
         "-I" + CSRC, "-I" + os.path.join(ROOT, "include")]


def compile_asm(src, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + FLAGS + [src, "-o", out], check=True)
    return open(out).read()


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return r.stdout.split("\n")[:len(names)]


def kernels(asm):
    """{mangled name: (instruction lines, {resource: value})} of every kernel of an assembly file."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^; Occupancy: \d+", asm, re.S | re.M):
        name, body = m.group(1), m.group(0)
        code = body.split(".section", 1)[0]
        # (a branch label carries the function's number in the file: .LBB7_2 -> .LBB_2)
        ins = [re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip()) for ln in code.split("\n")]
        ins = [ln for ln in ins if ln and not ln.endswith(":") and not ln.startswith(".")]
        res = {k: v for k, v in re.findall(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|private_segment_fixed_size)\s+(\d+)", body)}
        occ = re.search(r"; Occupancy: (\d+)", body)
        res["occupancy"] = occ.group(1) if occ else "?"
        out[name] = (ins, res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="harris.hip of the parent commit (compiled beside csrc/ for its headers)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        new = kernels(compile_asm(os.path.join(CSRC, "harris.hip"), os.path.join(tmp, "harris.s")))
        new8 = kernels(compile_asm(os.path.join(CSRC, "harris_u8.hip"), os.path.join(tmp, "harris_u8.s")))
        old = kernels(compile_asm(a.parent, os.path.join(tmp, "parent.s"))) if a.parent else None
    names = sorted(new) + sorted(new8)
    pretty = dict(zip(names, demangle(names)))
    want = ("harris_image_response", "harris_nms", "harris_list_kernel", "harris_keypoints_counted", "harris_u8_to_f32")
    print("kernel | VGPRs | SGPRs | scratch B | LDS B | waves/SIMD | instructions")
    for k in names:
        if not any(w in pretty[k] for w in want):
            continue
        ins, res = (new.get(k) or new8.get(k))
        print(f"{pretty[k]} | {res.get('next_free_vgpr')} | {res.get('next_free_sgpr')} | {res.get('private_segment_fixed_size')} | "
              f"{res.get('group_segment_fixed_size')} | {res['occupancy']} | {len(ins)}")
    if old is None:
        return 0
    print("\nf32 instantiations against the parent commit (instruction streams, comments and labels dropped):")
    bad = 0
    # (the f32 instantiation now names its pixel type: <1, 16, false> is <1, 16, false, float>)
    def norm(p):
        return p.replace(", float>(", ">(")
    new_by_name = {norm(pretty[k]): new[k] for k in new}
    for k in sorted(old):
        p = demangle([k])[0]
        if not any(w in p for w in ("harris_image_response_kernel", "harris_nms_tiled_kernel", "harris_nms_kernel", "harris_response_tiled_kernel")):
            continue
        got = new_by_name.get(norm(p))
        same = got is not None and got[0] == old[k][0] and got[1] == old[k][1]
        bad += not same
        print(f"{'identical' if same else 'DIFFERENT'} | {p} | {len(old[k][0])} instructions")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
