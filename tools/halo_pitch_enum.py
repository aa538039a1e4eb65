#!/usr/bin/env python3
"""z-pitch of the halo image in LDS for a brick of the halo convolution kernel (csrc/conv3d_halo.hpp: halo_pitch): host-side
enumeration of the bank conflicts of the A-fragment reads.

The kernel reads one 16-byte fragment per lane from the halo image (80-byte rows).  ds_read_b128 serves a wave in four fixed
16-lane groups over 64 banks, so a group is conflict-free iff the halo rows of its lanes are distinct mod 16 (lanes on the SAME
row read one address: a broadcast, not a conflict -- the pad rows of a brick all sit on voxel 0).  The kernel's greedy pass gives
lane l of a 32-row tile a voxel whose halo row is == l mod 16 wherever the tile holds that residue twice; this script replays
that pass for every tile of a brick and every candidate pitch and counts, per pitch,

    groups   16-lane groups (of 2 per tile: the upper wave half repeats the lower) with at least one conflict
    extra    serialised extra passes: sum over groups of (largest number of DISTINCT rows on one residue) - 1

and the LDS plan of the brick (the larger of the staging planes and the epilogue tile, plus the voxel table).

    python tools/halo_pitch_enum.py                 # the 2 x 10 x 10 Winograd brick, pitches 12..16
    python tools/halo_pitch_enum.py 4 8 8 --td      # the 4 x 8 x 8 brick (pitch 12: 0 conflicts)

--mfma16 replays the operand map of v_mfma_f32_16x16x32_bf16 instead (the `wz_mfma` = 16 form of the Winograd bricks): lane l of
a 16-row tile reads the 16-byte chunk l >> 4 of row l & 15, so a 16-lane group holds eight rows at chunk c and the OTHER eight at
chunk c + 1 (lanes {0-3, 12-15} with {20-27}; {4-11} with {16-19, 28-31}).  In 16-byte units a lane sits at
(row pitch * row + chunk) mod 16.  With an odd row pitch (80 bytes = 5) no assignment of rows to lanes is conflict-free: the
sixteen rows of a tile would have to take every residue, and then the set of the eight chunk-(c + 1) rows would have to map
onto itself under + 1.  With 96-byte rows (6) a row's position has the parity of its chunk, so a group is conflict-free iff
each of its two halves holds rows that are distinct mod 8 -- which no tap offset disturbs.  The kernel's greedy pass for this
form deals the rows of 32 consecutive voxels to four such halves by (residue mod 8, how many earlier rows share it); the
script replays it, per candidate z-pitch, and replays the weight tile (16 consecutive rows per tile, natural order).

    python tools/halo_pitch_enum.py --mfma16              # 2 x 10 x 10, pitches 12..16, and the weight tile
    python tools/halo_pitch_enum.py 4 8 8 --td --mfma16   # 4 x 8 x 8: 0 conflicts at every pitch (a z run is 8 consecutive rows)
"""
import argparse

LDKH = 40                                    # bf16 per LDS row (80 bytes)
LDKH16 = 48                                  # the same for the 16x16x32 form (96 bytes)
GROUPS = ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
          [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31])


def halo_row(r, by, bz, hy, pitch, xo):
    x, y, z = r // (by * bz), (r // bz) % by, r % bz
    return ((x + xo) * hy + (y + 1)) * pitch + (z + 1)


def assign_tile(rows, nvox, by, bz, hy, pitch, xo):
    """The kernel's greedy pass for one tile: slot -> brick row (None = pad row, which works on voxel 0)."""
    res = [halo_row(r if r < nvox else 0, by, bz, hy, pitch, xo) & 15 for r in rows]
    tab, left = [None] * 32, []
    seen = [0] * 16
    filled = [False] * 32
    for j, r in enumerate(rows):
        rank = seen[res[j]]
        seen[res[j]] += 1
        if rank < 2:
            tab[rank * 16 + res[j]], filled[rank * 16 + res[j]] = r, True
        else:
            left.append(r)
    empty = [j for j in range(32) if not filled[j]]
    for j, r in zip(empty, left):
        tab[j] = r
    return tab


def count(bx, by, bz, pitch, td, bnv=128):
    xo = 0 if td else 1
    hy = by + 2
    nvox = bx * by * bz
    mrows = (nvox + 127) // 128 * 128
    groups = extra = 0
    for t in range(mrows // 32):
        tab = assign_tile(list(range(t * 32, t * 32 + 32)), nvox, by, bz, hy, pitch, xo)
        hrows = [halo_row(r if r < nvox else 0, by, bz, hy, pitch, xo) for r in tab]
        for grp in GROUPS:
            by_res = {}
            for lane in grp:
                by_res.setdefault(hrows[lane] & 15, set()).add(hrows[lane])
            worst = max(len(v) for v in by_res.values())
            groups += worst > 1
            extra += worst - 1
    lrows = (bx + 2 * xo) * hy * pitch
    planes = (2 * lrows + 2 * 2 * bnv) * LDKH * 2
    stage = mrows * (128 + 8) * 4
    lds = max(planes, stage) + (mrows + 256) * 2
    return groups, extra, 2 * (mrows // 32), lds


def slot16(half, q):
    """16x16x32 form: slot (of 32) of the q-th row (q = residue mod 8) of half-group `half` (0..3): tile half >> 1; its lanes
    {0-3, 12-15} read one chunk (half even), its lanes {4-11} the next (half odd)."""
    i = 4 + q if half & 1 else (q if q < 4 else q + 8)
    return (half >> 1) * 16 + i


def assign_tile16(rows, nvox, by, bz, hy, pitch, xo):
    """The greedy pass of the 16x16x32 form for 32 consecutive brick rows: slot -> brick row."""
    res = [halo_row(r if r < nvox else 0, by, bz, hy, pitch, xo) & 7 for r in rows]
    tab, left = [None] * 32, []
    seen = [0] * 8
    filled = [False] * 32
    for j, r in enumerate(rows):
        rank = seen[res[j]]
        seen[res[j]] += 1
        if rank < 4:
            tab[slot16(rank, res[j])], filled[slot16(rank, res[j])] = r, True
        else:
            left.append(r)
    empty = [j for j in range(32) if not filled[j]]
    for j, r in zip(empty, left):
        tab[j] = r
    return tab


def conflicts16(tile_rows, row_chunks=LDKH16 * 2 // 16):
    """One 16-row tile on the 16x16x32 map: (groups with a conflict, extra passes) over the two 16-lane groups of a wave half
    (the upper half repeats the lower two chunks further on).  tile_rows[slot] is the LDS row of lane slot."""
    groups = extra = 0
    for grp in GROUPS:
        at = {}
        for lane in grp:
            row, chunk = tile_rows[lane & 15], lane >> 4
            at.setdefault((row_chunks * row + chunk) % 16, set()).add((row, chunk))
        worst = max(len(v) for v in at.values())
        groups += worst > 1
        extra += worst - 1
    return groups, extra


def count16(bx, by, bz, pitch, td, bnv=128, row_chunks=LDKH16 * 2 // 16):
    xo = 0 if td else 1
    hy = by + 2
    nvox = bx * by * bz
    mrows = (nvox + 127) // 128 * 128
    groups = extra = 0
    for t in range(mrows // 32):
        tab = assign_tile16(list(range(t * 32, t * 32 + 32)), nvox, by, bz, hy, pitch, xo)
        hrows = [halo_row(r if r < nvox else 0, by, bz, hy, pitch, xo) for r in tab]
        for h in range(2):
            g, e = conflicts16(hrows[h * 16:h * 16 + 16], row_chunks)
            groups += g
            extra += e
    lrows = (bx + 2 * xo) * hy * pitch
    planes = (2 * lrows + 2 * 2 * bnv) * row_chunks * 16
    stage = mrows * (128 + 8) * 4
    lds = max(planes, stage) + (mrows + 256) * 2
    return groups, extra, 4 * (mrows // 32), lds


def count16_weights(bnv=128, row_chunks=LDKH16 * 2 // 16):
    """The weight tile on the 16x16x32 map: 16 consecutive rows per tile, lane slot = row."""
    groups = extra = 0
    for t in range(bnv // 16):
        g, e = conflicts16(list(range(t * 16, t * 16 + 16)), row_chunks)
        groups += g
        extra += e
    return groups, extra, 2 * (bnv // 16)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("brick", nargs="*", type=int, default=[2, 10, 10])
    ap.add_argument("--td", action="store_true", help="2-D form (no halo along the first axis); default for the 2 x 10 x 10 brick")
    ap.add_argument("--mfma16", action="store_true", help="the operand map of the 16x16x32 MFMA on 96-byte rows (wz_mfma = 16)")
    a = ap.parse_args()
    bx, by, bz = a.brick
    td = a.td or a.brick == [2, 10, 10]
    print(f"brick {bx} x {by} x {bz} ({'2-D' if td else '3-D'} form), {bx * by * bz} rows"
          + (", 16x16x32 operand map, 96-byte rows" if a.mfma16 else ""))
    print("pitch  conflicting groups  extra passes  LDS bytes")
    for pitch in range(bz + 2, 17):
        g, e, n, lds = (count16 if a.mfma16 else count)(bx, by, bz, pitch, td)
        print(f"{pitch:5d}  {g:8d} of {n:3d}     {e:12d}  {lds:9d}{'' if lds <= 160 * 1024 else '  (over 160 KB)'}")
    if a.mfma16:
        for chunks in (5, 6):
            g, e, n = count16_weights(row_chunks=chunks)
            print(f"weight tile, {chunks * 16}-byte rows: {g} of {n} groups conflict, {e} extra passes")


if __name__ == "__main__":
    main()
