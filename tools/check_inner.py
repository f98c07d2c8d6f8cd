#!/usr/bin/env python3
"""Check every search kernel in the build's ISA (build/*-gfx950.s, kept by
the Makefile): search_kernel<P, NBV>, search_kernel_padc<P> and
search_kernel_padk<P, K>, for spill or memory traffic inside its innermost
loop, and print the per-nonce VALU count of each layout (-v).  Exit 1 if any
inner loop holds scratch/global/buffer ops; SGPR spills read back through
v_readlane (the generic padding-block kernel's) are counted and reported.
--header-versions: check header_versions_kernel<M> instead (the block-header
search, the bm_header_versions_inst unit), rows "hdrv1", "hdrv2", "hdrv4".  The
per-nonce code of an M-slot kernel is several basic blocks, because the rare
branch after each slot's compare splits it: every block of the per-nonce loop
from its header to its back edge is summed (the rare paths are laid out behind
the back edge; one that was not would show as a memory op, its atomic).  The
row gives VALU per nonce and per hash, the slow / fast split, the issue slots
per hash under DESIGN.md section 5's model, max(slow, (slow + fast) / 2), and the
v_readlane (SGPR spills read back), scratch and memory ops in that code.
--header-versions-hits: check header_versions_hits_kernel<M> (the version-rolling
share enumeration, the bm_header_versions_hits_inst unit), rows "hdrvh1",
"hdrvh2", "hdrvh4", as --header-versions does."""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_loops  # noqa: E402
from isa_mix import classify, inner_ops  # noqa: E402

BAD = re.compile(r"^(scratch_|buffer_|global_|flat_|s_buffer)")      # memory traffic: never in a loop
LANE = re.compile(r"^(v_readlane|v_writelane)")                       # SGPR spill via VGPR lanes
args = [a for a in sys.argv[1:] if not a.startswith("-")]
build = args[0] if args else os.path.join(ROOT, "distributed_bitcoin_minter_amd/csrc/build")
bad = 0
rows = []
HEADER_VERSIONS = "--header-versions" in sys.argv
HEADER_VERSIONS_HITS = "--header-versions-hits" in sys.argv
HEADER_ANY = HEADER_VERSIONS or HEADER_VERSIONS_HITS
for sfile in sorted(glob.glob(os.path.join(build, "*gfx950.s"))) if not HEADER_ANY else []:
    for name in isa_loops.kernels(sfile, "search_kernel"):
        m = re.search(r"search_kernel(_padc|_padk)?ILi(\d+)ELi(\d+)E(?:Li(\d+)E)?", name)
        if not m:
            continue
        kind, p, a = m.group(1), int(m.group(2)), int(m.group(3))
        tag = "c" if kind == "_padc" else f"k{a}" if kind == "_padk" else str(a)
        # the innermost loop (the deepest loop's biggest block: isa_mix.inner_ops)
        body = inner_ops(sfile, name)
        nbad = sum(1 for o, _ in body if BAD.match(o))
        nlane = sum(1 for o, _ in body if LANE.match(o))
        fast, slow = classify(body)
        rows.append((tag, p, fast + slow, slow, nbad, nlane))
        bad += nbad > 0


def loop_blocks(sfile, name):
    """The per-nonce loop's main line: the loop whose header block holds the
    most VALU, its blocks in layout order from the header to the back edge."""
    lines = isa_loops.kernels(sfile, name)[name]
    order, blocks, owner, cur, pending = [], {}, {}, None, None
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", l) or re.match(r"^; (%bb\.\d+):\s*(;.*)?$", l)
        if m:
            cur = pending = m.group(1)
            order.append(cur)
            blocks[cur] = []
            note = m.group(2) or ""
        elif pending and re.match(r"^\s*;", l):
            note = l
        else:
            note = ""
        if note and cur:
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            if h:
                owner[cur] = ".L" + h.group(1)
            elif "This Loop Header" in note or "This Inner Loop Header" in note:
                owner[cur] = cur
        if m or note:
            continue
        s = l.strip()
        if s and not s.startswith(";"):
            pending = None
        if cur and s and not s.startswith((";", ".")):
            blocks[cur].append((s.split()[0], s))
    valu = lambda b: sum(1 for o, _ in blocks[b] if o.startswith("v_"))
    head = max((b for b in order if owner.get(b) == b), key=valu)
    out = []
    for b in order[order.index(head):]:
        if owner.get(b) != head:
            break
        out.append(blocks[b])
        if any(o.startswith(("s_branch", "s_cbranch")) and t.split()[-1] == head for o, t in blocks[b]):
            return out
    raise SystemExit(f"{name}: no back edge found behind {head}")


VROWS = []
VUNITS = ([("bm_header_versions_inst", "header_versions_kernel", "hdrv")] if HEADER_VERSIONS else []) + \
         ([("bm_header_versions_hits_inst", "header_versions_hits_kernel", "hdrvh")] if HEADER_VERSIONS_HITS else [])
for sfile, kernel, tag in [(f, k, t) for u, k, t in VUNITS
                           for f in sorted(glob.glob(os.path.join(build, u + "*gfx950.s")))]:
    for name in isa_loops.kernels(sfile, kernel):
        slots = int(re.search(kernel + r"ILi(\d+)E", name).group(1))
        main = loop_blocks(sfile, name)
        body = [op for blk in main for op in blk]
        nbad = sum(1 for o, _ in body if BAD.match(o))
        nread = sum(1 for o, _ in body if o.startswith("v_readlane"))
        nlane = sum(1 for o, _ in body if LANE.match(o))
        fast, slow = classify(body)
        rows.append((f"{tag}{slots}", 0, fast + slow, slow, nbad, nlane))
        VROWS.append((tag, slots, fast, slow, nbad, nread, nlane - nread,
                      "+".join(str(sum(classify(blk))) for blk in main if sum(classify(blk)) >= 100)))
        bad += nbad > 0
for tag, slots, fast, slow, nbad, nread, nwrite, split in sorted(VROWS) if "-v" in sys.argv else []:
    valu = fast + slow
    print(f" 0:{tag}{slots} inner VALU={valu} slow={slow} fast={fast} VALU/hash={valu / slots:.1f} "
          f"slots/hash={max(slow, (slow + fast) / 2) / slots:.1f} mem={nbad} readlane={nread} writelane={nwrite} "
          f"blocks={split}")
rows_printed = [r for r in rows if not r[0].startswith("hdrv") or r[4]]
for tag, p, valu, slow, nbad, nlane in sorted(rows_printed, key=lambda r: (len(r[0]), r[0], r[1])):
    if nbad or "-v" in sys.argv:
        print(f"{p:2d}:{tag:3s} inner VALU={valu} slow={slow} mem={nbad} lane-spill={nlane}")
print(f"{len(rows)} kernels checked, {bad} with scratch/memory ops in the inner loop, "
      f"{sum(1 for r in rows if r[5])} with v_readlane/v_writelane in it")
sys.exit(1 if bad else 0)
