"""The LDS paddings of nhwc.hip (NhwcBlockCfg::MS, NhwcStripCfg::CS) by brute force, with the bank rule of ds_write_b32 /
ds_read_b32 on gfx950: bank = dword address mod 32, conflicts counted per 32-lane half, equal addresses broadcast.

    python tools/nhwc_lds_banks.py

Per edge: the best (stores + reads, stores, reads, MS) candidates - the conflict degree of the staging stores (thread t
stores channel t % CB of pixel t / CB at (t % CB) * MS + t / CB) and of the pass-1 reads (lane = column c of map g1 reads
g1 * MS + c) - and the same for MS = CodeletCfg's MAP_LDS. A model, not a hardware count."""
from collections import Counter
def deg(addrs):
    worst = 0
    for half in (addrs[:32], addrs[32:]):
        c = Counter(a % 32 for a in set(half))
        worst = max(worst, max(c.values()))
    return worst
cfg = {14: (4, 17, 238, 32), 16: (4, 17, 272, 32), 28: (2, 33, 924, 16), 32: (2, 33, 1056, 8)}
for N, (G, S, MAP, CB) in cfg.items():
    best = []
    lim = min(MAP + 70, 65536 // 4 // CB)
    for MS in range(MAP, lim + 1):
        w = max(deg([(t % CB) * MS + t // CB for t in range(w0, w0 + 64)]) for w0 in range(0, 64 * CB // G, 64))
        r = deg([((l // N) * MS + (l % N)) if l // N < G else 0 for l in range(64)])
        best.append((w + r, w, r, MS))
    best.sort()
    print(N, best[:4], "MAP_LDS itself:", [b for b in best if b[3] == MAP])
# the 56 x 56 strips: [CB = 4][R * 56 = 448] floats, CS floats per channel; reads are one channel, consecutive columns
for CS in range(448, 448 + 33):
    w = max(deg([(t % 4) * CS + t // 4 for t in range(w0, w0 + 64)]) for w0 in range(0, 256, 64))
    if w == 1:
        print(56, "first conflict-free CS:", CS)
        break
