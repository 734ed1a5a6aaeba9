#!/usr/bin/env python3
"""The gfx950 listing of the matrix-core SSD kernel, block by block (no device needed).

Compiles csrc/ws_march_mfma.hip with -S for gfx950 (or reads a listing given with --listing) and prints, for every
basic block that holds at least --min-mfma MFMAs (default 8: the tile loops of the two roles):

  * its instructions by class (VALU / MFMA / LDS read / LDS write / VMEM / SALU / s_waitcnt / s_nop / other);
  * for every LDS read, the number of instructions between it and the s_waitcnt that covers it.  LDS operations
    return in order, so `s_waitcnt lgkmcnt(N)` retires all but the youngest N of the block's outstanding ones.  Every
    block is taken to start with nothing outstanding.  That holds for the step's blocks because `__syncthreads` waits
    `lgkmcnt(0)` in front of the barrier on the loop's back edge; a read still in flight from a predecessor block
    would make a wait retire fewer of the block's own reads than is counted here;
  * the pairs of neighbouring MFMAs (in MFMA order) that write one accumulator, with the instructions between them;
  * the kernel's VGPR / AGPR / SGPR / scratch / spill figures.

    python tools/mfma_listing.py                    # this tree
    python tools/mfma_listing.py --csrc DIR         # another tree's csrc (a parent export)
    python tools/mfma_listing.py --listing FILE.s   # a listing made elsewhere

A report for profiles/mfma_pipeline/README.md, not a test.
"""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-x", "hip", "--cuda-device-only", "-S"]

LABEL = re.compile(r"^([.\w$]+):")
LGKM = re.compile(r"lgkmcnt\((\d+)\)")
META = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
        "group_segment_fixed_size")


def compile_listing(csrc, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False)
    out.close()
    try:
        subprocess.check_call([hipcc] + FLAGS + extra + [os.path.join(csrc, "ws_march_mfma.hip"), "-o", out.name])
        with open(out.name) as f:
            return f.read()
    finally:
        os.remove(out.name)


def classify(op):
    if op.startswith("v_mfma"):
        return "MFMA"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op == "s_nop":
        return "s_nop"
    if op.startswith("ds_"):
        return "LDS read" if ("read" in op or "load" in op or "permute" in op or "swizzle" in op) else "LDS write"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def blocks_of(text):
    """(kernel, label, [(opcode, operands)]) for every basic block of every kernel in the listing."""
    kernel, label, cur = None, None, []
    for raw in text.splitlines():
        line = raw.split(";")[0].rstrip()
        if not line.strip():
            continue
        m = LABEL.match(line)
        if m:
            if cur:
                yield kernel, label, cur
            cur = []
            label = m.group(1)
            if not label.startswith("."):
                kernel = label
            continue
        s = line.strip()
        if s.startswith("."):
            continue
        parts = s.split(None, 1)
        op, args = parts[0], parts[1] if len(parts) > 1 else ""
        cur.append((op, args))
        if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
            yield kernel, label, cur
            cur, label = [], (label or "") + "+"
    if cur:
        yield kernel, label, cur


def report_block(kernel, label, ins):
    counts = {}
    for op, _ in ins:
        c = classify(op)
        counts[c] = counts.get(c, 0) + 1
    print("block %s of %s: %d instructions" % (label, kernel, len(ins)))
    print("  by class: " + ", ".join("%s %d" % (k, counts[k]) for k in
                                     ("VALU", "MFMA", "LDS read", "LDS write", "VMEM", "SALU", "s_waitcnt", "s_nop", "other") if k in counts))
    # the in-order queue of the block's own LDS (and scalar-memory) operations
    queue, dist, waits = [], [], []
    for i, (op, args) in enumerate(ins):
        c = classify(op)
        if c in ("LDS read", "LDS write") or op.startswith(("s_load", "s_buffer_load")):
            queue.append((i, c, op))
        elif c == "s_waitcnt":
            m = LGKM.search(args)
            if not m:
                continue
            n = int(m.group(1))
            keep = min(n, len(queue))
            done, queue = queue[:len(queue) - keep], queue[len(queue) - keep:]
            reads = [(i - j - 1, op2) for j, c2, op2 in done if c2 == "LDS read"]
            dist += reads
            waits.append((i, n, [d for d, _ in reads]))
    ds = sorted(d for d, _ in dist)
    if ds:
        print("  LDS reads covered by a wait in the block: %d; instructions between read and wait: min %d, median %s, max %d"
              % (len(ds), ds[0], statistics.median(ds), ds[-1]))
        print("    distances: " + " ".join(str(d) for d in ds))
    print("  LDS reads still outstanding at the block's end: %d" % sum(1 for _, c, _ in queue if c == "LDS read"))
    print("  lgkm waits (position: count -> distances of the reads it retires):")
    for pos, n, r in waits:
        print("    %4d: lgkmcnt(%d) -> %s" % (pos, n, " ".join(map(str, r)) if r else "-"))
    mf = [(i, args.split(",")[0].strip()) for i, (op, args) in enumerate(ins) if op.startswith("v_mfma")]
    pairs = [(a, b, d) for (a, d), (b, e) in zip(mf, mf[1:]) if d == e]
    print("  MFMA order (accumulator @ position): " + " ".join("%s@%d" % (d, i) for i, d in mf))
    if pairs:
        print("  neighbouring MFMAs on one accumulator: " + ", ".join("%s (%d instructions between)" % (d, b - a - 1) for a, b, d in pairs))
    else:
        print("  neighbouring MFMAs on one accumulator: none")
    return ds


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=os.path.join(ROOT, "stereo_reconstruction_amd", "csrc"))
    ap.add_argument("--listing", help="read this listing instead of compiling")
    ap.add_argument("--min-mfma", type=int, default=8)
    ap.add_argument("--flag", action="append", default=[], help="an extra compiler flag (repeatable)")
    a = ap.parse_args()
    text = open(a.listing).read() if a.listing else compile_listing(a.csrc, a.flag)
    shown = 0
    for kernel, label, ins in blocks_of(text):
        if sum(1 for op, _ in ins if op.startswith("v_mfma")) >= a.min_mfma:
            report_block(kernel, label, ins)
            print()
            shown += 1
    print("%d blocks with at least %d MFMAs; s_waitcnt in the whole listing: %d" % (shown, a.min_mfma, len(re.findall(r"^\s*s_waitcnt", text, re.M))))
    for key in META:
        vals = re.findall(r"\.%s:\s*(\d+)" % key, text)
        if vals:
            print("  .%s: %s" % (key, ", ".join(vals)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
