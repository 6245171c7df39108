#!/usr/bin/env python
"""Host model of csrc/conv2_wgrad_rows.hip's LDS image: which byte of y1 every staged 16-B
chunk holds, which bytes every ds_read_b64_tr_b16 lane of every wave, step and split reads,
and the schedule of the ring.  Checks, for a list of (images, rows_per_split):

* every fragment lane reads the pixel chunk the GEMM wants (input row 2 oh + kh, pixel
  2 ow + kw, channels 16 t + 4 pcol ..) or the zero cell past the split end;
* the row is resident when its step computes (issued before, not yet overwritten) and no
  piece lands on a slot a running or coming step still reads;
* LDS bank conflicts of the transposed reads: per 32-lane half, the lanes' 8-byte reads
  must fall on 64 distinct banks (bank = (addr / 4) % 64); prints the worst multiplicity,
  apart for the reads of a split's last step that mix the zero cell with real rows.

    python scripts/lds_conflicts_conv2_wgrad_rows.py
"""
import sys

D, SLOT, LO, ROWS = 24, 5120, 2560, 64
CELLS = D * 40
ZERO = D * SLOT


def f_of(v):
    return ((v >> 1) & 1) | (((v >> 3) & 1) << 1)


def piece(Q, J0, kh):
    """(LDS byte address -> (plane, J, input row, pixel, chunk)) of the 64 lanes of piece Q."""
    jr, k = divmod(Q, 5)
    J = J0 + jr
    out = {}
    for lane in range(64):
        sc = 8 * k + (lane >> 3)
        plane, w20 = divmod(sc, 20)
        e, usw = divmod(w20, 10)
        u = usw ^ (J & 1)
        c = (lane & 7) ^ (f_of(9 * J + u) << 1)
        img, oh = divmod(J, 9)
        out[(jr % D) * SLOT + k * 1024 + lane * 16] = (plane, img, 2 * oh + kh, 2 * u + e, c)
    return out


def check(N, rows):
    Mred = N * 81
    nsplit = (Mred + rows - 1) // rows
    worst, worst_tail = 1, 1        # all rows inside the split / some past its end
    for split in range(nsplit):
        r_begin, r_end = split * rows, min(Mred, (split + 1) * rows)
        nst = (r_end - r_begin + ROWS - 1) // ROWS
        J0, Jlast = r_begin // 9, (r_end - 1) // 9
        jhi = lambda st: (min(r_end, r_begin + ROWS * (st + 1)) - 1) // 9
        jlo = lambda st: (r_begin + ROWS * st) // 9
        for kh in range(4):
            lds = {}                              # byte address of a 16-B chunk -> content

            def issue(Qa, Qb, keep_from):
                for Q in range(Qa, Qb):
                    for a, v in piece(Q, J0, kh).items():
                        old = lds.get(a)
                        # a slot is reused only when no running / coming step reads its row
                        assert old is None or old[1] * 9 + (old[2] - kh) // 2 < keep_from, (N, rows, split, Q)
                        lds[a] = v

            q3 = 5 * (min(Jlast, J0 + D - 1) - J0 + 1)
            issue(0, q3, J0)
            Qn = q3
            for st in range(nst):
                if st + 1 < nst:
                    q1 = max(Qn, 5 * (jhi(st + 1) - J0 + 1))
                    q3 = max(q1, 5 * (min(Jlast, jlo(st) + D - 1) - J0 + 1))
                    # issued while step st computes: model them as landing AFTER its reads
                    pending = (Qn, q3, jlo(st))
                    Qn = q3
                else:
                    pending = None
                for half in range(2):
                    for kw in range(4):
                        for second in range(2):
                            for plane in range(2):
                                for t in range(4):
                                    addrs, tail = [], False
                                    for lane in range(64):
                                        g, q, pcol = lane >> 4, (lane >> 2) & 3, lane & 3
                                        r = ROWS * st + 32 * half + 8 * g + q + 4 * second
                                        m = r_begin + r
                                        if m < r_end:
                                            J, ow = divmod(m, 9)
                                            h = kw >> 1
                                            cell = ((J - J0) % D) * 40 + ((ow + h) ^ (J & 1))
                                            f = f_of(m + h)
                                            a = cell * 128 + (kw & 1) * 1280 + 8 * pcol
                                        else:
                                            f, a, tail = 0, CELLS * 128 + 8 * pcol, True
                                        a += plane * LO + ((t ^ f) << 5)
                                        addrs.append(a)
                                        if m < r_end:
                                            img, oh = divmod(J, 9)
                                            want = (plane, img, 2 * oh + kh, 2 * ow + kw, 2 * t + (pcol >> 1))
                                            assert lds.get(a & ~15) == want, (N, rows, split, kh, st, kw, lane)
                                            assert (a & 15) == 8 * (pcol & 1)
                                        else:
                                            assert ZERO <= a - plane * LO < ZERO + 128
                                    for hw in range(2):
                                        banks = {}
                                        for a in addrs[32 * hw:32 * hw + 32]:
                                            for b in ((a >> 2) & 63, ((a >> 2) + 1) & 63):
                                                banks.setdefault(b, set()).add(a)
                                        w = max(len(s) for s in banks.values())
                                        if tail:
                                            worst_tail = max(worst_tail, w)
                                        else:
                                            worst = max(worst, w)
                if pending:
                    issue(*pending)
    return worst, worst_tail


def main():
    cases = [(1, 128), (9, 704), (18, 128), (37, 704), (37, 352), (24, 352), (64, 704), (7, 1024), (5, 64)]
    bad = 0
    for N, rows in cases:
        w, wt = check(N, rows)
        print(f"N={N:3d} rows_per_split={rows:4d}: addressing and ring schedule ok, worst tr-read bank "
              f"multiplicity {w} ({'conflict-free' if w == 1 else 'CONFLICTS'}); reads that mix in the zero "
              f"cell (a split's last step): {wt}")
        bad += w != 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
