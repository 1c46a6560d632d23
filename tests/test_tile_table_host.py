"""The tile table of a camera launch (och::plan::tile_table in csrc/och_tiles.cpp),
built without a device by a small C++ program compiled from that file.

The render kernels read one descriptor per wave in place of working out their
tile; a wrong descriptor puts a pixel in the wrong place or leaves it out.  Every
entry is compared here with a pure-Python restatement of the mapping (view,
first column, slice row and frame row of lane 0, the whole-tile-inside bit), and
the table as a whole with the properties a launch needs: every frame pixel of
the shard exactly once, padding waves none.  The same program runs once under
AddressSanitizer and UBSan as a stand-alone binary: the builder indexes by
computed sizes.
"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "octree_ray_tracing_amd" / "csrc"

ROWS, INSIDE, EMPTY, SPLIT = 1 << 28, 1 << 29, 1 << 30, 1 << 31
E_INVALID = -1

# table W H views row_chunk shard n_shards slice_rows block supertiles quiet
#       n_map [map] n_order [order] n_tasks [tasks]
# -> status grid n [entries]      (quiet: without the entries)
DRIVER = r'''
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>
#include "och_tiles.h"
template <class T>
static std::vector<T> rd()
{
    size_t n;
    std::cin >> n;
    std::vector<T> v(n);
    for (auto &x : v) {
        long long t;
        std::cin >> t;
        x = (T)t;
    }
    return v;
}
int main()
{
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd != "table") return 2;
        och::plan::TileGeometry g;
        int quiet;
        std::cin >> g.width >> g.height >> g.n_views >> g.row_chunk >> g.shard >> g.n_shards >> g.slice_rows >> g.block >>
            g.supertiles >> quiet;
        const std::vector<int32_t> map = rd<int32_t>();
        const std::vector<uint32_t> order = rd<uint32_t>(), tasks = rd<uint32_t>();
        g.chunk_map = map.empty() ? nullptr : map.data();
        std::vector<uint64_t> table;
        uint32_t grid = 0;
        const char *why = nullptr;
        const int st = och::plan::tile_table(g, order.empty() ? nullptr : order.data(), (uint32_t)order.size(),
                                             tasks.empty() ? nullptr : tasks.data(), (uint32_t)tasks.size(), table, grid,
                                             &why);
        if (st != 0 && (!why || !*why)) return 3;          // a refusal names its reason
        printf("%d %u %zu", st, grid, table.size());
        if (!quiet)
            for (uint64_t e : table) printf(" %llu", (unsigned long long)e);
        printf("\n");
    }
    return 0;
}
'''


def command(W, H, views, rc, shard, n, slice_rows, block, supertiles, cmap=(), order=(), tasks=(), quiet=0):
    arr = lambda a: f"{len(a)} " + " ".join(str(int(x)) for x in a)
    return (f"table {W} {H} {views} {rc} {shard} {n} {slice_rows} {block} {supertiles} {quiet} "
            f"{arr(cmap)} {arr(order)} {arr(tasks)}\n")


def run_driver(exe, commands):
    run = subprocess.run([str(exe)], input="".join(commands), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
    out = []
    for line in run.stdout.splitlines():
        w = line.split()
        st, grid, n = int(w[0]), int(w[1]), int(w[2])
        out.append((st, grid, n, np.array(w[3:], dtype=np.uint64)))
    assert len(out) == len(commands)
    return out


def compile_driver(tmp, name, cc, flags):
    src, exe = tmp / "tile_table_host.cpp", tmp / name
    src.write_text(DRIVER)
    run = subprocess.run([*cc, "-std=c++17", "-O1", "-g", "-Wall", *flags, f"-I{CSRC}", str(src),
                          str(CSRC / "och_tiles.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("tile_table_host")


@pytest.fixture(scope="module")
def driver(tmp):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = compile_driver(tmp, "plain", [cxx], [])
    return lambda commands: run_driver(exe, commands)


# ------------------------------------------------------- the mapping, restated

def ceil_div(a, b):
    return -(-a // b)


def shard_rows(H, rc, n):
    return ceil_div(ceil_div(H, rc), n) * rc


def deal_maps(chunk_shard, n):
    """The per-shard chunk maps of a row deal (och_gpu_set_row_deal): each shard's chunks in
    frame order, padded with -1 to the largest shard's count."""
    mine = [[c for c, s in enumerate(chunk_shard) if s == sh] for sh in range(n)]
    mx = max(1, max(len(m) for m in mine))
    return [m + [-1] * (mx - len(m)) for m in mine], mx


def frame_row(srow, H, rc, shard, n, cmap):
    """Frame row of slice row srow, H (no row) for a padding chunk."""
    chunk = srow // rc
    g = cmap[chunk] if cmap else chunk * n + shard
    return H if g < 0 else g * rc + srow % rc


def xcd_block(b, nb, group):
    """Workgroup b of the launch -> logical workgroup: runs of `group` consecutive logical
    workgroups per XCD (workgroups go round-robin over 8 XCDs); the grid's tail stays put."""
    span = 8 * group
    if group == 0 or b >= nb - nb % span:
        return b
    return ((b // 8 // group) * 8 + b % 8) * group + (b // 8) % group


def logical_tile(wave, W, slice_rows, views, supertiles):
    """(view, tile column, tile row) of logical wave `wave`, or None past the last view."""
    tiles_x, tiles_y = ceil_div(W, 8), ceil_div(slice_rows, 8)
    if supertiles:
        sx = ceil_div(tiles_x, 8)
        per_view = sx * ceil_div(tiles_y, 8) * 64
        view, t = divmod(wave, per_view)
        st, sub = divmod(t, 64)
        tx, ty = (st % sx) * 8 + sub % 8, (st // sx) * 8 + sub // 8
    else:
        per_view = tiles_x * tiles_y
        view, t = divmod(wave, per_view)
        ty, tx = divmod(t, tiles_x)
    return (view, tx, ty) if view < views else None


def launch_waves(W, slice_rows, views, block, supertiles, order):
    """The logical wave of every wave of the launch, in launch order (None: past the frame's waves)."""
    tiles_x, tiles_y = ceil_div(W, 8), ceil_div(slice_rows, 8)
    per_view = ceil_div(tiles_x, 8) * ceil_div(tiles_y, 8) * 64 if supertiles else tiles_x * tiles_y
    waves, wpb = per_view * views, block // 64
    blocks = ceil_div(waves, wpb)
    group = 64 // wpb if supertiles and order is None else 0
    out = []
    for b in range(blocks):
        blk = int(order[b]) if order is not None else xcd_block(b, blocks, group)
        out += [blk * wpb + w if blk * wpb + w < waves else None for w in range(wpb)]
    return out, blocks


def check_table(geo, order, got):
    """Every entry against the restated mapping; then coverage, by running the kernel's
    per-lane arithmetic (CameraSource::locate) over the table."""
    W, H, views, rc, shard, n, slice_rows, block, supertiles, cmap = geo
    st, grid, n_entries, table = got
    waves, blocks = launch_waves(W, slice_rows, views, block, supertiles, order)
    assert st == 0 and grid == blocks and n_entries == len(waves) == table.size, (geo, st, grid, n_entries)
    cover = np.zeros((views, slice_rows, W), dtype=np.int32)
    for k, wave in enumerate(waves):
        w0, w1 = int(table[k]) & 0xFFFFFFFF, int(table[k]) >> 32
        assert not w0 & SPLIT
        tile = logical_tile(wave, W, slice_rows, views, supertiles) if wave is not None else None
        pixels = []                                         # (srow, col) of the tile inside the frame
        if tile is not None:
            view, tx, ty = tile
            pixels = [(s, c) for s in range(ty * 8, ty * 8 + 8) for c in range(tx * 8, tx * 8 + 8)
                      if c < W and s < slice_rows and frame_row(s, H, rc, shard, n, cmap) < H]
        if not pixels:
            assert w0 & EMPTY, (geo, k, hex(w0))            # a padding wave covers nothing
            continue
        assert not w0 & EMPTY, (geo, k, hex(w0))
        col0, e_view, srow0, row0 = w0 & 0xFFFF, (w0 >> 16) & 15, w1 >> 16, w1 & 0xFFFF
        assert (e_view, col0, srow0) == (view, tx * 8, ty * 8), (geo, k)
        assert bool(w0 & INSIDE) == (len(pixels) == 64 and not w0 & ROWS), (geo, k, hex(w0))
        if rc % 8 == 0 or (n == 1 and not cmap):
            assert not w0 & ROWS, (geo, k)                  # the tile lies in one chunk, or slice row = row
        if not w0 & ROWS:
            assert row0 == frame_row(srow0, H, rc, shard, n, cmap), (geo, k)
        # the kernel's view of the entry, lane by lane
        for lane in range(64):
            c, s = col0 + lane % 8, srow0 + lane // 8
            if w0 & INSIDE:
                r = row0 + lane // 8
            else:
                if c >= W or s >= slice_rows:
                    continue
                r = frame_row(s, H, rc, shard, n, cmap) if w0 & ROWS else row0 + lane // 8
                if r >= H:
                    continue
            assert r == frame_row(s, H, rc, shard, n, cmap) and c < W and s < slice_rows and r < H, (geo, k, lane)
            cover[e_view, s, c] += 1
    want = np.zeros_like(cover)
    for s in range(slice_rows):
        if frame_row(s, H, rc, shard, n, cmap) < H:
            want[:, s, :] = 1
    assert np.array_equal(cover, want), geo                 # every frame pixel of the shard exactly once


def deals(H, rc, n, deal_chunks):
    """Round-robin (no map) and, for n > 1, a weighted deal by och_deal_chunks."""
    yield None
    if n == 1:
        return
    n_chunks = ceil_div(H, rc)
    rng = np.random.default_rng(1000 * H + n)
    costs = rng.uniform(0.5, 4.0, n_chunks).astype(np.float32)
    weights = rng.uniform(0.5, 2.0, n).astype(np.float32)
    out = deal_chunks(costs, n, weights)
    yield out.tolist()


def geometries(deal_chunks):
    rc = 8
    for W in (1, 7, 8, 9, 63, 64, 65):
        for H in (1, 3, 8, 9, 17):
            for n in (1, 2, 3, 8):
                for deal in deals(H, rc, n, deal_chunks):
                    maps, mx = deal_maps(deal, n) if deal else (None, 0)
                    slice_rows = mx * rc if deal else shard_rows(H, rc, n)
                    for shard in range(n):
                        for views in (1, 2, 3):
                            yield W, H, views, rc, shard, n, slice_rows, tuple(maps[shard]) if deal else ()


def test_every_entry_and_the_coverage_of_small_frames(driver, ort):
    from octree_ray_tracing_amd.tracer import deal_chunks
    rng = np.random.default_rng(20261019)
    cases, commands = [], []
    for W, H, views, rc, shard, n, slice_rows, cmap in geometries(deal_chunks):
        for block in (64, 128, 256):
            blocks = ceil_div(ceil_div(W, 8) * ceil_div(slice_rows, 8) * views, block // 64)
            # natural, planned (a random permutation), grouped per XCD (supertiles)
            for supertiles, order in ((0, None), (0, rng.permutation(blocks)), (1, None)):
                cases.append(((W, H, views, rc, shard, n, slice_rows, block, supertiles, cmap), order))
                commands.append(command(W, H, views, rc, shard, n, slice_rows, block, supertiles, cmap,
                                        order if order is not None else ()))
    for (geo, order), got in zip(cases, driver(commands)):
        check_table(geo, order, got)


def test_tiles_that_straddle_row_chunks(driver):
    """Row chunks that are no multiple of 8 on several shards: a tile's rows come from several
    chunks, so its lanes map their own rows (the rows flag), unless the rows happen to be consecutive."""
    cases, commands = [], []
    for rc, n in ((3, 2), (1, 3), (5, 2), (12, 2)):
        for H in (17, 40):
            for shard in range(n):
                geo = (20, H, 2, rc, shard, n, shard_rows(H, rc, n), 64, 0, ())
                cases.append(geo)
                commands.append(command(*geo))
    flagged = 0
    for geo, got in zip(cases, driver(commands)):
        check_table(geo, None, got)
        flagged += int(np.count_nonzero(got[3] & np.uint64(ROWS)))
    assert flagged > 0


def test_split_waves_name_their_task_row_and_tile(driver):
    """A split order (bit 31 entries): the wave's entry holds its task row and the index, behind
    the launch's entries, of its heavy tile's descriptor."""
    W, H = 24, 16                                           # 3 x 2 tiles
    tasks = np.full(3 * 65, 0xFFFFFFFF, dtype=np.uint32)
    tasks[0], tasks[65], tasks[130] = 4, 4, 1               # rows 0, 1: tile 4; row 2: tile 1
    order = [SPLIT | 0, SPLIT | 1, SPLIT | 2, 0, 2, 3, 5]
    (plain, got) = driver([command(W, H, 1, 8, 0, 1, H, 64, 0), command(W, H, 1, 8, 0, 1, H, 64, 0, (), order, tasks)])
    st, grid, n, table = got
    assert (st, grid, n) == (0, 7, 10)
    for k, (row, tile) in enumerate(((0, 4), (1, 4), (2, 1))):
        w0, w1 = int(table[k]) & 0xFFFFFFFF, int(table[k]) >> 32
        assert w0 == SPLIT | row and w1 == 7 + k
        assert table[w1] == plain[3][tile]
    assert [int(x) for x in table[3:7]] == [int(plain[3][t]) for t in (0, 2, 3, 5)]
    # refused: a task row past the table, a tile past the frame, a block of more than one wave
    bad = driver([command(W, H, 1, 8, 0, 1, H, 64, 0, (), [SPLIT | 3, 0, 1, 2, 3, 4, 5], tasks),
                  command(W, H, 1, 8, 0, 1, H, 64, 0, (), order, np.where(tasks == 1, 6, tasks)),
                  command(W, H, 1, 8, 0, 1, H, 128, 0, (), [SPLIT | 0, 0, 1, 2], tasks)])
    assert [b[0] for b in bad] == [E_INVALID] * 3 and all(b[2] == 0 for b in bad)


def test_the_packing_range(driver):
    """3840 x 2160 with OCH_MAX_VIEWS views fits; past 65 535 columns or rows is refused, as is
    an order that is no order of the grid."""
    out = driver([command(3840, 2160, 8, 8, 0, 1, 2160, 64, 0, quiet=1),
                  command(65535, 8, 1, 8, 0, 1, 8, 64, 0, quiet=1),
                  command(65536, 8, 1, 8, 0, 1, 8, 64, 0, quiet=1),
                  command(8, 65536, 1, 65536, 0, 1, 65536, 64, 0, quiet=1),
                  command(8, 70000, 1, 8, 0, 2, 35000, 64, 0, quiet=1),
                  command(8, 8, 9, 8, 0, 1, 8, 64, 0, quiet=1),
                  command(16, 8, 1, 8, 0, 1, 8, 64, 0, (), [0, 2], quiet=1),
                  command(16, 8, 1, 8, 0, 1, 8, 64, 0, (), [0], quiet=1)])
    assert [o[0] for o in out] == [0, 0, E_INVALID, E_INVALID, E_INVALID, E_INVALID, E_INVALID, E_INVALID]
    assert out[0][1] == 480 * 270 * 8 and out[0][2] == 480 * 270 * 8


def test_under_address_and_undefined_sanitizers(tmp):
    """The same program as a stand-alone sanitized binary over a sample of the cases above
    (straddling chunks, a deal with padding chunks, a split order, refusals)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if Path(hipcc).exists():
        cc, flags = [hipcc], ["-x", "c++"] + [f for s in san for f in ("-Xarch_host", s)]
    else:
        cxx = shutil.which("g++") or shutil.which("clang++")
        if cxx is None:
            pytest.skip("no C++ compiler")
        cc, flags = [cxx], san
    exe = compile_driver(tmp, "sanitized", cc, flags)
    tasks = np.full(65, 0xFFFFFFFF, dtype=np.uint32)
    tasks[0] = 3
    commands = [command(65, 17, 3, 8, 1, 3, 8, 256, 1),
                command(63, 17, 2, 8, 0, 2, 16, 128, 0, (2, -1)),
                command(20, 40, 2, 3, 1, 2, 21, 64, 0),
                command(24, 16, 1, 8, 0, 1, 16, 64, 0, (), [SPLIT | 0, 5, 4, 2, 1, 0], tasks),
                command(24, 16, 1, 8, 0, 1, 16, 64, 0, (), [SPLIT | 7, 5, 4, 2, 1, 0], tasks),
                command(65536, 8, 1, 8, 0, 1, 8, 64, 0, quiet=1),
                command(3840, 2160, 8, 8, 0, 1, 2160, 64, 1, quiet=1)]
    out = run_driver(exe, commands)
    assert [o[0] for o in out] == [0, 0, 0, 0, E_INVALID, E_INVALID, 0]
