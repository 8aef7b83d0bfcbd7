"""TEST-ONLY CPU models of the structure of csrc/mlm.hip, in the kernels' own partition: the two-pass compaction of the selected tokens
(per-block counts of 256 tokens, a prefix over the blocks, ballot ranks inside a block) and the per-(row, lane) folding of a vocabulary
sweep (lane = absolute group of four columns mod 64, online maximum / sum in float32), with the chunk list of `functional.mlm_vocab_chunks`
restated."""
import numpy as np

F32 = np.float32


def place(flags, cap):
    """flags: bool [T] in token order -> (sel [cap] with -1 behind the kept ones, kept, selected), as mlm_count_kernel + mlm_place_kernel
    place them: token i of block b = i // 256 lands at sum(counts[:b]) + (selected tokens of the block in front of i)"""
    flags = np.asarray(flags, dtype=bool)
    T = flags.shape[0]
    nb = (T + 255) // 256
    counts = [int(flags[256 * b: 256 * (b + 1)].sum()) for b in range(nb)]
    sel = np.full(cap, -1, dtype=np.int32)
    for b in range(nb):
        base = sum(counts[:b])
        for w in range(4):                                     # the four waves of the block
            lo = 256 * b + 64 * w
            lanes = flags[lo: lo + 64]
            woff = int(flags[256 * b: lo].sum())
            for lane in np.flatnonzero(lanes):
                pos = base + woff + int(lanes[:lane].sum())    # popcount of the ballot below the lane
                if pos < cap:
                    sel[pos] = lo + lane
    total = sum(counts)
    return sel, min(total, cap), total


def vocab_chunks(V, rows, chunk_bytes, planes=False):
    vc = max(128, chunk_bytes // (rows * (8 if planes else 4)) // 128 * 128)
    V8 = V // 8 * 8
    chunks = [(v0, min(vc, V8 - v0), 0) for v0 in range(0, V8, vc)]
    if V8 != V:
        chunks.append((V - 8, 8, 8 - (V - V8)))
    return chunks


def _rescale(st, mx):
    if mx > st[0] or mx != mx:
        st[1] = F32(st[1] * np.exp(F32(st[0] - mx), dtype=F32))
        st[0] = mx


def _add(st, x, col):
    st[1] = F32(st[1] + np.exp(F32(x - st[0]), dtype=F32))
    if st[3] < 0 or x > st[2] or (x != x and st[2] == st[2]):
        st[2], st[3] = x, col


def fold_row(x, chunks):
    """x: float32 [V] logits of one row (bias included) -> (lse, argmax) from 64 lane states folded chunk by chunk as
    mlm_xent_stats_kernel does and merged as mlm_xent_rows_kernel does (the butterfly's sum order)"""
    x = np.asarray(x, dtype=F32)
    lanes = [[F32(-np.inf), F32(0), F32(-np.inf), -1] for _ in range(64)]
    with np.errstate(invalid="ignore", over="ignore"):
        for v0, cols, skip in chunks:
            if skip == 0 and v0 % 4 == 0 and cols % 4 == 0:
                for g in range(cols // 4):
                    c = v0 + 4 * g
                    st = lanes[(c // 4) % 64]
                    v = x[c: c + 4]
                    a = v[0] if (v[0] != v[0] or v[0] > v[1]) else v[1]     # max_keep_nan of the pairs (0, 1) and (2, 3), then of both
                    b = v[2] if (v[2] != v[2] or v[2] > v[3]) else v[3]
                    mx = a if (a != a or a > b) else b
                    _rescale(st, mx)
                    for q in range(4):
                        _add(st, v[q], c + q)
            else:
                for j in range(skip, cols):
                    c = v0 + j
                    st = lanes[c % 64]
                    _rescale(st, x[c])
                    _add(st, x[c], c)
        M = lanes[0][0]
        for st in lanes[1:]:
            M = M if (M != M or M > st[0]) else st[0]
        terms = [F32(0) if st[0] == -np.inf else F32(st[1] * np.exp(F32(st[0] - M), dtype=F32)) for st in lanes]
        for o in (32, 16, 8, 4, 2, 1):                         # __shfl_xor butterfly: lane l takes l + (l ^ o)
            terms = [F32(terms[l] + terms[l ^ o]) for l in range(64)]
        best = None
        for st in lanes:
            if st[3] < 0:
                continue
            if best is None:
                best = (st[2], st[3])
                continue
            bv, bi = best
            ov, oi = st[2], st[3]
            if ov != ov or bv != bv:
                take = (ov != ov) and (bv == bv or oi < bi)
            else:
                take = ov > bv or (ov == bv and oi < bi)
            if take:
                best = (ov, oi)
        return F32(M + np.log(terms[0], dtype=F32)), (best[1] if best else -1)
