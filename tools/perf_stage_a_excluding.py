#!/usr/bin/env python3
"""GPU timing of stage A with excluded words at BASELINE configs[2]'s shape (10,000 x 30,000, packed once): per
direction and for the both-directions call, in one session, the plain call, the sets call with n_exclude = 0 (the
same launches: any difference beyond run-to-run spread is a bug), 100 excluded winners, and 1,000 and 10,000
vocabulary words (words read off the search windows of the first rows; the 10,000 are more than k_exclude stages in
LDS).  Event-timed on the device around each blocking call; best of `reps`.  The excluded runs are checked: no
excluded word is returned, and the winners differ from the plain ones.

k_exclude alone: run this tool under `rocprofv3 --kernel-trace --stats` and read k_exclude against k_extract in the
kernel statistics (one launch per excluded call; the list length of each is in the order of the calls above).

usage: tools/perf_stage_a_excluding.py [rows] [length] [reps]"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "open-msspe-design_amd"))
import numpy as np
import torch
import msspe_amd as m

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
length = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
SEG, STRIDE, WIN, K = 500, 250, 50, 13
g = m.synth.aligned_genomes(rows, length)
eng = m.Engine(0)
d = eng.put_rows_packed(g)
mm = max(1, min(10, -(-rows // 50)))
opt = m.KmerOpt(SEG, STRIDE, WIN, K, 1000, mm)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def vocabulary(direction, want):
    """`want` distinct words of the direction's index, read off the windows of the first rows."""
    seen, out = set(), []
    for row in g:
        text = bytes(row)
        for part in range((length - SEG) // STRIDE + 1):
            c0 = part * STRIDE + (SEG - WIN if direction else 0)
            for p in range(WIN - K + 1):
                w = text[c0 + p:c0 + p + K]
                if w.strip(b"ACGT"):
                    continue
                w = (w.translate(COMP)[::-1] if direction else w).decode()
                if w not in seen:
                    seen.add(w)
                    out.append(w)
                    if len(out) == want:
                        return out
    return out


def timed(call):
    best, out = None, None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return round(best, 3), out


lists, plain = {}, {}
for direction in (0, 1):
    line = {"direction": direction}
    line["plain_ms"], (w, f) = timed(lambda: eng.kmer_candidates_packed(d, rows, length, opt, direction))
    plain[direction] = w
    line["winners"] = len(w)
    line["n_exclude_0_ms"], (w0, f0) = timed(lambda: eng.kmer_candidates_packed(d, rows, length, opt, direction, exclude=[]))
    assert w0 == w and f0.tolist() == f.tolist(), "n_exclude = 0 is not the plain call"
    vocab = vocabulary(direction, 10000)
    lists[direction] = {"winners_100": w[:100], "vocab_1000": vocab[:1000], "vocab_10000": vocab}
    for name, excl in lists[direction].items():
        ms, (w2, _) = timed(lambda: eng.kmer_candidates_packed(d, rows, length, opt, direction, exclude=excl))
        assert not set(w2) & set(excl), f"{name}: an excluded word was returned"
        assert w2 != w, f"{name}: the exclusions changed nothing"
        line[f"{name}_ms"], line[f"{name}_n"] = ms, len(excl)
    print(json.dumps(line), flush=True)

line = {"direction": "both"}
line["plain_ms"], both = timed(lambda: eng.kmer_candidates_both_packed(d, rows, length, opt))
assert both[0][0] == plain[0] and both[1][0] == plain[1]
line["n_exclude_0_ms"], both0 = timed(lambda: eng.kmer_candidates_both_packed(d, rows, length, opt, exclude_fwd=[], exclude_rev=[]))
assert both0[0][0] == plain[0] and both0[1][0] == plain[1]
for name in lists[0]:
    ms, got = timed(lambda: eng.kmer_candidates_both_packed(d, rows, length, opt, exclude_fwd=lists[0][name],
                                                            exclude_rev=lists[1][name]))
    for direction in (0, 1):
        assert not set(got[direction][0]) & set(lists[direction][name]), f"both, {name}: an excluded word was returned"
    line[f"{name}_ms"] = ms
print(json.dumps(line), flush=True)
eng.device_free(d)
eng.close()
