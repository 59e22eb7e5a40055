"""csrc/flx_queue_build.h on the CPU: the index arithmetic of the queue build (logic.hip: k_queue_build), run by tests/queue_build_cpu.cpp the
way the kernel runs it -- block counts and segment totals, persistent blocks over runs of segments, waves over 256-path tiles, four membership
bytes per lane -- and compared with the stable compaction numpy.cumsum gives: a path's slot in a list is the list's starting counter plus the
number of paths with a smaller id in it.

The program is built with AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone executable (nothing is loaded into Python); its
buffers have exactly the lists' sizes, so an index that is off by one is a report, not a silent write.
"""
import os
import shutil
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = 7
TILE = 256
SEG = 64 * 256              # paths per segment
FREE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("queue_build") / "queue_build_cpu")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "queue_build_cpu.cpp"), "-o", out]
    assert shutil.which("g++"), "the suite builds its native code with g++"
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    return out


def members(n, mix, seed):
    """membership bytes: bit0 raygen, bit1 shadow, bits 2..4 material list 0..5 (a path of the raygen list has no material list)"""
    rng = np.random.default_rng(seed)
    if mix == "random":
        ray = rng.random(n) < 0.2
        ml = np.where(ray, 0, rng.integers(0, 6, n))
        sh = (~ray) & (rng.random(n) < 0.8)
    elif mix == "one-list":             # every path in the glossy list, nothing anywhere else
        ray = np.zeros(n, bool); sh = np.zeros(n, bool); ml = np.full(n, 2)
    elif mix == "all-of-them":          # every path in the shadow list AND a material list: all four bytes of every lane, aligned 16-byte stores
        ray = np.zeros(n, bool); sh = np.ones(n, bool); ml = np.full(n, 1)
    elif mix == "shadow-empty":
        ray = rng.random(n) < 0.5
        ml = np.where(ray, 0, rng.integers(1, 6, n)); sh = np.zeros(n, bool)
    elif mix == "empty":
        ray = np.zeros(n, bool); sh = np.zeros(n, bool); ml = np.zeros(n, int)
    elif mix == "runs":                 # adversarial: long runs that start and end off the tile and segment boundaries, a lone member at each end
        i = np.arange(n)
        ray = (i % 1021) < 500
        ml = np.where(ray, 0, 1 + (i // 333) % 5)
        sh = (i % 7 == 3) & ~ray
        ray[0] = True; ml[0] = 0
        if n > 1:
            ray[-1] = False; ml[-1] = 5; sh[-1] = True
    elif mix == "every-fourth":         # one byte per lane, a different one from tile to tile
        i = np.arange(n)
        ray = (i % 4) == ((i // TILE) % 4)
        ml = np.where(ray, 0, np.where(i % 4 == 3, 4, 0)); sh = (i % 4 == 1) & ~ray
    else:
        raise AssertionError(mix)
    return (ray.astype(np.uint8) | (sh.astype(np.uint8) << 1) | (ml.astype(np.uint8) << 2)).astype(np.uint8)


def grid_of(n, num_cus, per_cu):
    """(blocks, blocks that share a segment): at most num_cus x per_cu blocks; fewer segments than that are split in 2, 4, 8 or 16 parts"""
    segments, cap, parts = -(-(-(-n // 256)) // 64), num_cus * per_cu, 1
    while parts < 16 and segments * 2 * parts <= cap:
        parts *= 2
    return min(segments * parts, cap), parts


def in_list(m, l):
    return (m & 1) != 0 if l == 0 else (m & 2) != 0 if l == 1 else (m >> 2) == l - 1


def run(exe, tmp_path, m, snapshot, num_cus, per_cu):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([m.size, num_cus, per_cu] + list(snapshot), np.uint32).tobytes())
        f.write(m.tobytes())
    r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout
    out = np.fromfile(fout, np.uint32)
    grid, parts, counters, at, queues = int(out[0]), int(out[1]), out[2:2 + LISTS], 2 + LISTS, []
    for _ in range(LISTS + 2):
        n = int(out[at]); queues.append(out[at + 1:at + 1 + n]); at += 1 + n
    assert at == out.size
    return (grid, parts), counters, queues


def check(exe, tmp_path, n, mix, snapshot=(0,) * LISTS, num_cus=2, per_cu=2, seed=1):
    m = members(n, mix, seed)
    grid, counters, queues = run(exe, tmp_path, m, snapshot, num_cus, per_cu)
    sets = [in_list(m, l) for l in range(LISTS)]
    mat = (m >> 2) != 0
    sets += [mat, mat | ((m & 1) != 0)]
    for l, s in enumerate(sets):
        base = snapshot[l] if l < LISTS else 0
        slot = base + np.cumsum(s) - 1                       # the stable compaction: where path i goes if it is in the list
        want = np.full(base + int(s.sum()), FREE, np.uint32)
        want[slot[s]] = np.nonzero(s)[0]
        assert queues[l].size == want.size, f"list {l}: {queues[l].size} entries, {want.size} expected"
        bad = np.nonzero(queues[l] != want)[0]
        assert bad.size == 0, f"list {l}: {bad.size} slots differ, first slot {bad[0]}: {queues[l][bad[0]]} for {want[bad[0]]}"
        if l < LISTS:
            assert int(counters[l]) == base + int(s.sum()), f"counter of list {l}: {counters[l]}"
    return grid


# one tile + 1 = 257; one segment +- 1; with 2 x 2 persistent blocks and 9 segments a block's share is 3 segments: +- 1 path around it;
# 5 segments on 4 blocks: shares of 2, 2, 1 and nothing for the last; up to 2 segments the four blocks split them between them (grid_of)
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1000, SEG - 1, SEG, SEG + 1, 3 * SEG - 1, 3 * SEG, 3 * SEG + 1, 9 * SEG - 77, 5 * SEG - 100,
          12 * SEG - 1, 12 * SEG, 12 * SEG + 1]      # four blocks with exactly three segments each, one path less, one more (then four each, the last block one)


@pytest.mark.parametrize("n", COUNTS)
def test_every_path_lands_in_its_stable_compaction_slot(exe, tmp_path, n):
    assert check(exe, tmp_path, n, "random", seed=n) == grid_of(n, 2, 2)


@pytest.mark.parametrize("mix", ["one-list", "all-of-them", "shadow-empty", "empty", "runs", "every-fourth"])
@pytest.mark.parametrize("n", [257, 1000, SEG + 1, 5 * SEG - 100])
def test_list_mixes(exe, tmp_path, mix, n):
    check(exe, tmp_path, n, mix)


@pytest.mark.parametrize("n", [1, 257, SEG + 1, 9 * SEG - 77])
def test_lists_append_behind_non_zero_counters(exe, tmp_path, n):
    # (odd bases: a lane whose four paths are all members then starts off a 16-byte boundary)
    check(exe, tmp_path, n, "random", snapshot=(5, 1, 1000, 3, 0, 77, 2), seed=7)
    check(exe, tmp_path, n, "all-of-them", snapshot=(0, 3, 6, 0, 0, 0, 0))


def test_segments_shared_by_blocks_and_one_block_for_everything(exe, tmp_path):
    assert check(exe, tmp_path, 5 * SEG - 100, "random", num_cus=256, per_cu=4) == (80, 16)  # a small wavefront: 16 blocks share a segment, a tile per wave
    assert check(exe, tmp_path, 5 * SEG - 100, "runs", num_cus=5, per_cu=4) == (20, 4)       # ... four blocks, four tiles per wave
    assert check(exe, tmp_path, 257, "random", num_cus=256, per_cu=4) == (16, 16)            # one segment, two tiles of it in use
    assert check(exe, tmp_path, 5 * SEG - 100, "random", num_cus=1, per_cu=1) == (1, 1)      # one block walks all five segments
    assert check(exe, tmp_path, 5 * SEG - 100, "runs", num_cus=3, per_cu=1) == (3, 1)        # shares of 2, 2, 1
