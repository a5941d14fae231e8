"""The search behind tests/jpegenc_cases.py's FAT_BLOCK: a pixel hill-climb for the 8 x 8 gray block with the most entropy-coded
bits at quality 100, coded behind an all-black block (prediction -1024, so the DC difference has size 11).  The objective is the
restatement's own bit count (tests/jpegenc_np.py).  The entropy kernel's stuffing loop takes a third pass from 129 whole bytes on:
1032 bits with the 7 bits a block can inherit, so 1025 of its own.

    python tests/tools/jpeg_fat_block.py [--steps 4000] [--batch 192] [--seed 7]      (prints the best block as a literal)
"""
import argparse
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

import jpegenc_np as ref  # noqa: E402

PRED = -1024        # the DC of an all-black block at quality 100


def exact_bits(z):
    w = ref.BitWriter()
    ref.encode_block(w, [int(v) for v in z], PRED, ref.huff_codes(ref.DC_LUMA), ref.huff_codes(ref.AC_LUMA))
    return 8 * len(bytes(w.out).replace(b"\xff\x00", b"\xff")) + w.n


def coefficients(blocks):
    """[n][8][8] uint8 -> [n][64]"""
    return ref.coefficients(np.concatenate(list(blocks), axis=1), 100)[0, :, 0, :]


def climb(steps, batch, seed):
    rng = np.random.default_rng(seed)
    ac = ref.huff_codes(ref.AC_LUMA)
    dc = ref.huff_codes(ref.DC_LUMA)
    ac_cost = np.array([0] + [ac[s][1] + s for s in range(1, 11)])          # run 0: what a busy block pays per coefficient
    dc_cost = np.array([dc[s][1] + s for s in range(12)])

    def estimate(z):
        size = np.ceil(np.log2(np.abs(z[:, 1:]) + 1)).astype(int)
        dsize = np.ceil(np.log2(np.abs(z[:, 0] - PRED) + 1)).astype(int)
        return np.where(dsize == 11, ac_cost[size].sum(axis=1) + dc_cost[dsize], 0)       # only blocks whose DC difference has size 11

    start = (rng.random((batch, 8, 8)) < 0.6).astype(np.uint8) * 255                       # brighter than 128 on average: DC >= 0
    z = coefficients(start)
    k = int(np.argmax(estimate(z)))
    best, best_bits = start[k].copy(), exact_bits(z[k])
    for step in range(steps):
        cand = np.repeat(best[None], batch, axis=0)
        for i in range(batch):
            for _ in range(int(rng.integers(1, 4))):
                y, x = rng.integers(0, 8, size=2)
                kind = rng.integers(0, 4)
                cand[i, y, x] = (0, 255, int(rng.integers(0, 256)), int(np.clip(int(cand[i, y, x]) + rng.integers(-12, 13), 0, 255)))[kind]
        z = coefficients(cand)
        k = int(np.argmax(estimate(z) + rng.random(batch) * 0.5))
        bits = exact_bits(z[k])
        if bits >= best_bits and z[k, 0] - PRED >= 1024:
            if bits > best_bits:
                print(f"step {step}: {bits} bits", file=sys.stderr)
            best, best_bits = cand[k].copy(), bits
    return best, best_bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    block, bits = climb(a.steps, a.batch, a.seed)
    print(f"# {bits} bits behind a black block; {(bits + 7) // 8} whole bytes with a carry of 7")
    print("FAT_BLOCK = [" + ",\n             ".join("[" + ", ".join(f"{v:3d}" for v in row) + "]" for row in block) + "]")


if __name__ == "__main__":
    main()
