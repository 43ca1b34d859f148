"""k_encode_tiles' workgroup order (model.h enc_block_decode, through mon_debug_encode_block: the one function host and kernel share).

The kernel takes its level and its sample partition from this decode and indexes the level table, the tile image and the feature rows with them: a decode
that leaves [0, L) x [0, 16) is an illegal access, one that visits a pair twice leaves another pair's features unwritten.  So, without a GPU: for every
L in 1..16 the 16 L workgroups of a grid row visit every (level, partition) exactly once -- with 1..3 batch chunks (grid rows; the kernel's partition of the
batch is 16 chunk + partition) every (level, partition, chunk) -- and for L = 16 the workgroups that share an XCD label x (b mod 8: b and b + 8) walk the four
levels 4 (x div 2) .. 4 (x div 2) + 3 with the eight partitions 8 (x mod 2) .. 8 (x mod 2) + 7 each, which is what puts a quarter of the tile image and half
of the positions into one L2.  L = 8 and L = 4 get four levels x four / two partitions per label; every other L keeps level = b div 16."""
import ctypes as C

import pytest

WG_PER_LEVEL = 16
N_XCD = 8


def decode(pkg, b, L):
    level, part = C.c_uint32(0xffffffff), C.c_uint32(0xffffffff)
    assert pkg.diag_lib().mon_debug_encode_block(b, L, C.byref(level), C.byref(part)) == 0, (b, L)
    return level.value, part.value


@pytest.mark.parametrize("L", range(1, 17))
def test_every_level_partition_and_chunk_is_walked_exactly_once(pkg, L):
    for chunks in (1, 2, 3):
        seen = {}
        for y in range(chunks):
            for b in range(WG_PER_LEVEL * L):
                level, part = decode(pkg, b, L)
                assert level < L and part < WG_PER_LEVEL, (L, b, level, part)
                key = (level, y * WG_PER_LEVEL + part)
                assert key not in seen, (L, chunks, b, y, key, seen[key])
                seen[key] = (b, y)
        assert len(seen) == L * WG_PER_LEVEL * chunks


@pytest.mark.parametrize("L", (4, 8, 16))
def test_a_label_walks_four_levels_and_a_share_of_the_partitions(pkg, L):
    ppx = L // 2                     # partitions of a level per label
    per = WG_PER_LEVEL // ppx        # labels that share a group of four levels
    for x in range(N_XCD):
        pairs = sorted(decode(pkg, b, L) for b in range(x, WG_PER_LEVEL * L, N_XCD))
        want = [(lv, p) for lv in range(4 * (x // per), 4 * (x // per) + 4) for p in range((x % per) * ppx, (x % per) * ppx + ppx)]
        assert pairs == want, (L, x, pairs)
    for b in range(WG_PER_LEVEL * L - N_XCD):
        assert decode(pkg, b, L)[0] // 4 == decode(pkg, b + N_XCD, L)[0] // 4 == (b % N_XCD) // per, (L, b)


@pytest.mark.parametrize("L", (1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15))
def test_other_level_counts_keep_the_plain_order(pkg, L):
    for b in range(WG_PER_LEVEL * L):
        assert decode(pkg, b, L) == (b // WG_PER_LEVEL, b % WG_PER_LEVEL), (L, b)


def test_blocks_and_level_counts_outside_the_grid_are_refused(pkg):
    level, part = C.c_uint32(0), C.c_uint32(0)
    dl = pkg.diag_lib()
    for b, L in ((16, 1), (256, 16), (0, 0), (0, 17), (0, -1)):
        assert dl.mon_debug_encode_block(b, L, C.byref(level), C.byref(part)) != 0, (b, L)
    assert dl.mon_debug_encode_block(0, 1, None, C.byref(part)) != 0 and dl.mon_debug_encode_block(0, 1, C.byref(level), None) != 0
