"""The launch planners of the C-ABI layer (och::plan in csrc/och_plan.cpp), called
without a device from a small C++ program compiled from that file and its header.

Frames do not depend on the launch order, so no GPU parity test can see a wrong
order; this file is the pin.  Layer 1 asserts properties and hand-checkable
cases from first principles, and runs its cases once more through the same
program built with AddressSanitizer and UBSan as a stand-alone binary: the
planners index by computed sizes.  Layer 2 compares the planners word for word with
tests/golden/plan_parent.npz: the outputs of the loop bodies these planners
were lifted from (och_api.cpp at commit 8ac5967: the stable sort :1599-1601,
plan_shape :1419-1442, the heavy-tile choice and split packing :1471-1474 and
:1488-1525, the XCD grouping :1608-1627, the chunk-cost spread :1776-1784), run
over the inputs that golden_cases() regenerates from the seed in the file.
"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

CSRC = Path(__file__).resolve().parents[1] / "octree_ray_tracing_amd" / "csrc"
GOLDEN = Path(__file__).resolve().parent / "golden" / "plan_parent.npz"
GOLDEN_SEED = 20261019
IDLE = 0xFFFFFFFF
LONG_PCT = 30            # kSplitRayPct

# Reads commands from stdin, prints one line per output array (length, then the words).
DRIVER = r'''
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include "och_plan.h"
using namespace och::plan;
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
static void pr(const std::vector<uint32_t> &v)
{
    printf("%zu", v.size());
    for (uint32_t x : v) printf(" %u", x);
    printf("\n");
}
int main()
{
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "by_cost") {
            pr(by_cost(rd<uint32_t>()));
        } else if (cmd == "shape") {
            int mode;
            std::cin >> mode;
            std::vector<uint32_t> o = rd<uint32_t>();
            shape(o, mode);
            pr(o);
        } else if (cmd == "group") {
            uint32_t tx, ty, block;
            std::cin >> tx >> ty >> block;
            pr(group_by_xcd(rd<uint32_t>(), tx, ty, block));
        } else if (cmd == "pack") {
            int S;
            std::cin >> S;
            const std::vector<int> cnt = rd<int>();
            if (cnt.size() != 64) return 3;
            pr(pack_split_tile(cnt.data(), S));
        } else if (cmd == "split") {      // the plan is shape(by_cost(costs), mode), as och_gpu_plan_views makes it
            int W, rows, pct, S, mode;
            std::cin >> W >> rows >> pct >> S >> mode;
            const std::vector<uint16_t> push = rd<uint16_t>();
            const std::vector<uint32_t> c = rd<uint32_t>();
            const std::vector<uint32_t> bc = by_cost(c);
            std::vector<uint32_t> o = bc;
            shape(o, mode);
            const Split s = split_order(push, W, rows, bc, o, c, pct, S);
            pr(s.order);
            pr(s.tasks);
            pr({s.tiles, s.extra});
        } else if (cmd == "spread") {     // floats as their bits
            int n_views, W, H, per_block, row_chunk;
            std::cin >> n_views >> W >> H >> per_block >> row_chunk;
            const std::vector<float> f = spread_chunk_costs(rd<uint32_t>(), n_views, W, H, (uint32_t)per_block, row_chunk);
            std::vector<uint32_t> bits(f.size());
            if (!f.empty()) std::memcpy(bits.data(), f.data(), f.size() * 4);
            pr(bits);
        } else {
            return 2;
        }
    }
    return 0;
}
'''


def command(head, *arrays):
    """One command of the driver's input: the head, then each array as its length and words."""
    return " ".join([head] + [f"{len(a)} " + " ".join(str(int(x)) for x in a) for a in arrays]) + "\n"


def run_driver(exe, commands):
    """Run the commands in one process; the output arrays, in order, as uint32."""
    run = subprocess.run([str(exe)], input="".join(commands), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    out = [np.array(line.split()[1:], dtype=np.uint64).astype(np.uint32) for line in run.stdout.splitlines()]
    for line, a in zip(run.stdout.splitlines(), out):
        assert int(line.split()[0]) == a.size
    return out


def compile_driver(tmp, name, cc, flags):
    src, exe = tmp / "plan_host.cpp", tmp / name
    src.write_text(DRIVER)
    run = subprocess.run([*cc, "-std=c++17", "-O1", "-g", "-Wall", *flags, f"-I{CSRC}", str(src),
                          str(CSRC / "och_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("plan_host")


@pytest.fixture(scope="module")
def planner(tmp):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = compile_driver(tmp, "plain", [cxx], [])
    return lambda commands: run_driver(exe, commands)


def is_permutation(a, n):
    return a.size == n and np.array_equal(np.sort(a), np.arange(n, dtype=np.uint32))


# ------------------------------------------------------------------ layer 1

def test_by_cost_is_the_stable_costliest_first_order(planner):
    c = np.random.default_rng(1).integers(0, 6, 300)                  # many ties
    (got,) = planner([command("by_cost", c)])
    assert np.array_equal(got, np.argsort(-c, kind="stable"))
    assert planner([command("by_cost", [])])[0].size == 0


def test_shape(planner):
    rng = np.random.default_rng(2)
    modes, cases = (0, 1, 10, 50, 99, 100), []
    for n in (0, 1, 2, 7, 100):
        o = rng.permutation(n)
        cases += [(n, mode, o) for mode in modes]
    outs = planner([command(f"shape {mode}", o) for _, mode, o in cases])
    for (n, mode, o), got in zip(cases, outs):
        assert is_permutation(got, n), (n, mode)
        if mode == 0:
            assert np.array_equal(got, o)
        elif mode < 100:
            head = n * mode // 100
            assert np.array_equal(got[:head], o[:head]), (n, mode)
            assert np.all(np.diff(got[head:].astype(np.int64)) > 0), (n, mode)
    o = np.array([3, 0, 4, 1, 2])
    (got,) = planner([command("shape 100", o)])
    assert got.tolist() == [o[0], o[4], o[1], o[3], o[2]]


def xcd_list(b, tiles_x, tiles_y, block):
    """The XCD list of workgroup b: its first tile's 64x64-pixel supertile, dealt round-robin."""
    tile = b * (block // 64)
    view, t = tile // (tiles_x * tiles_y), tile % (tiles_x * tiles_y)
    stx, sty = -(-tiles_x // 8), -(-tiles_y // 8)
    return ((view * sty + (t // tiles_x) // 8) * stx + (t % tiles_x) // 8) % 8


GROUP_CASES = [(1, 1, 1, 64), (8, 8, 1, 64), (240, 135, 2, 64), (65, 37, 2, 128), (65, 37, 2, 256)]


def test_group_by_xcd(planner):
    rng = np.random.default_rng(3)
    orders = [rng.permutation(-(-tx * ty * views // (block // 64))) for tx, ty, views, block in GROUP_CASES]
    outs = planner([command(f"group {tx} {ty} {block}", o) for (tx, ty, _, block), o in zip(GROUP_CASES, orders)])
    for (tx, ty, views, block), o, got in zip(GROUP_CASES, orders, outs):
        n = o.size
        assert is_permutation(got, n), (tx, ty, block)
        lst_in, lst_out = xcd_list(o, tx, ty, block), xcd_list(got.astype(np.int64), tx, ty, block)
        for x in range(8):      # the input's relative order within each list
            assert np.array_equal(got[lst_out == x], o[lst_in == x]), (tx, ty, block, x)
        full = 8 * min(np.count_nonzero(lst_in == x) for x in range(8))   # slots before any list runs dry
        assert np.array_equal(lst_out[:full], np.arange(full) % 8), (tx, ty, block)
    # 8x8 tiles are one supertile: list 0 holds all, the fallback serves every other slot from it
    assert np.array_equal(outs[1], orders[1])
    assert outs[0].tolist() == [0]


def pack_cases():
    rng = np.random.default_rng(4)
    ragged = rng.integers(0, 400, 64)
    ragged[rng.permutation(64)[:40]] = -1
    one_long = np.full(64, 10)
    one_long[27] = 1000
    single = np.full(64, -1)
    single[5] = 77
    return {"equal": np.full(64, 50), "zero": np.zeros(64, int), "one_long": one_long,
            "all_long": rng.integers(900, 1000, 64), "ragged": ragged, "single": single}


def check_packing(cnt, S, waves):
    """Every property of one tile's waves; returns the number of waves."""
    assert waves.size % 64 == 0
    mx = max(0, int(cnt.max()))
    seen = {}
    for w, wave in enumerate(waves.reshape(-1, 64)):
        busy = wave != IDLE
        assert busy.any() and busy[:int(busy.sum())].all(), "at most 64 tasks, then idle lanes"
        for word in wave[busy].tolist():
            pixel, seg, lg = word & 63, (word >> 6) & 15, word >> 10
            seen.setdefault(pixel, []).append((w, seg, lg))
    assert sorted(seen) == [l for l in range(64) if cnt[l] >= 0], "present pixels, and no absent one"
    for pixel, tasks in seen.items():
        is_long = int(cnt[pixel]) * 100 > LONG_PCT * mx
        lanes = S if is_long else 1
        assert len({w for w, _, _ in tasks}) == 1, "one wave per ray"
        assert [seg for _, seg, _ in tasks] == list(range(lanes)), (pixel, tasks)
        assert {lg for _, _, lg in tasks} == {S.bit_length() - 1 if is_long else 0}, (pixel, tasks)
    return waves.size // 64


def test_pack_split_tile(planner):
    cases = [(name, S, cnt) for name, cnt in pack_cases().items() for S in (2, 4, 8, 16)]
    outs = {(name, S): got for (name, S, _), got in zip(cases, planner([command(f"pack {S}", cnt) for _, S, cnt in cases]))}
    n_waves = {(name, S): check_packing(cnt, S, outs[name, S]) for name, S, cnt in cases}
    assert n_waves["all_long", 16] == 16 and not np.any(outs["all_long", 16] == IDLE)    # 16 full waves
    for S in (2, 4, 8, 16):
        assert n_waves["equal", S] == S              # 64 long rays of S lanes fill S waves
        assert n_waves["zero", S] == 1               # mx = 0: nothing is long
        assert n_waves["single", S] == 1
        assert n_waves["one_long", S] == 2           # 63 short lanes + S do not fit one wave


def test_pack_split_tile_places_costly_rays_first(planner):
    # the long ray's lane estimate 1000 / S still exceeds the short rays' 10: it leads the first wave
    cnt = pack_cases()["one_long"]
    (got,) = planner([command("pack 4", cnt)])
    assert got[:4].tolist() == [27 | s << 6 | 2 << 10 for s in range(4)]
    assert got[4:64].tolist() == [l for l in range(64) if l != 27][:60]     # ties keep pixel order
    assert got[64:67].tolist() == [61, 62, 63] and np.all(got[67:] == IDLE)


@pytest.mark.parametrize("per_block", [1, 2, 4])
@pytest.mark.parametrize("H,row_chunk", [(289, 8), (20, 3)])
def test_spread_chunk_costs(planner, H, row_chunk, per_block):
    W, n_views = 100, 1
    tiles = n_views * -(-W // 8) * -(-H // 8)
    assert tiles % 2 == 1                            # no multiple of per_block 2 or 4: a short last workgroup
    n_blocks = -(-tiles // per_block)
    c = np.random.default_rng(5).integers(0, 1 << 20, n_blocks)
    (bits,) = planner([command(f"spread {n_views} {W} {H} {per_block} {row_chunk}", c)])
    got = bits.view(np.float32).astype(np.float64)
    assert got.size == -(-H // row_chunk)
    in_block = np.minimum(tiles, (np.arange(n_blocks) + 1) * per_block) - np.arange(n_blocks) * per_block
    want = float(np.sum(c.astype(np.float64) * in_block / per_block))
    # each output is one float32 rounding of a double sum; the double sums' own error is far below that
    assert abs(got.sum() - want) <= want * (2.0 ** -24 + 1e-12)


def split_inputs(costs, push_of_tile, tiles_x=16, tiles_y=9):
    push = np.zeros((tiles_y * 8, tiles_x * 8), np.int64)
    for t, cnt in push_of_tile.items():
        ty, tx = divmod(t, tiles_x)
        push[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = np.asarray(cnt).reshape(8, 8)
    return push.ravel(), np.asarray(costs)


def test_split_order(planner):
    rng = np.random.default_rng(6)
    n, S, mode = 16 * 9, 4, 10
    costs = rng.integers(50, 200, n)
    costs[37], costs[90] = 1000, 900                              # exactly two tiles reach 80 % of the costliest
    cnt = {37: np.full(64, 50), 90: rng.integers(0, 300, 64)}
    push, costs = split_inputs(costs, cnt)
    order, tasks, counts, by_cost, plan, w37, w90 = planner([
        command(f"split 128 72 80 {S} {mode}", push, costs), command("by_cost", costs),
        command(f"shape {mode}", np.argsort(-costs, kind="stable")), command(f"pack {S}", cnt[37]),
        command(f"pack {S}", cnt[90])])
    assert by_cost[:2].tolist() == [37, 90]
    waves = (w37.size + w90.size) // 64
    assert counts.tolist() == [2, waves - 2]                      # heavy tiles, extra = waves - heavy tiles
    assert order[:waves].tolist() == [1 << 31 | row for row in range(waves)]
    rows = tasks.reshape(waves, 65)
    assert rows[:, 0].tolist() == [37] * (w37.size // 64) + [90] * (w90.size // 64)    # by_cost order of the tiles
    assert np.array_equal(rows[:, 1:].ravel(), np.concatenate([w37, w90]))
    assert np.array_equal(order[waves:], plan[(plan != 37) & (plan != 90)])               # plan order, heavy absent


def test_split_order_cap_and_zero_threshold(planner):
    flat = np.full(16 * 9, 7)                                     # every tile reaches 100 % of the costliest
    push, costs = split_inputs(flat, {t: np.full(64, 3) for t in range(16 * 9)})
    small_push, small_costs = split_inputs(np.full(9, 7), {t: np.full(64, 3) for t in range(9)}, 3, 3)
    capped, one, off = [planner([cmd]) for cmd in (command("split 128 72 100 2 10", push, costs),
                                                   command("split 24 24 100 2 10", small_push, small_costs),
                                                   command("split 128 72 0 2 10", push, costs))]
    assert capped[2].tolist() == [9, 9]                           # n / 16 tiles, the first of by_cost; 2 waves each
    assert sorted(set(capped[1].reshape(-1, 65)[:, 0].tolist())) == list(range(9))
    assert capped[0].size == 18 + (144 - 9)
    assert one[2].tolist() == [1, 1] and one[0].size == 2 + 8     # max(1, 9 / 16) = 1
    assert off[2].tolist() == [0, 0] and off[0].size == 0 and off[1].size == 0   # threshold 0: no split plan


def layer1_commands():
    """The inputs of the layer-1 tests above, from the same seeds."""
    cmds = [command("by_cost", np.random.default_rng(1).integers(0, 6, 300)), command("by_cost", [])]
    rng = np.random.default_rng(2)
    for n in (0, 1, 2, 7, 100):
        o = rng.permutation(n)
        cmds += [command(f"shape {mode}", o) for mode in (0, 1, 10, 50, 99, 100)]
    rng = np.random.default_rng(3)
    cmds += [command(f"group {tx} {ty} {block}", rng.permutation(-(-tx * ty * views // (block // 64))))
             for tx, ty, views, block in GROUP_CASES]
    cmds += [command(f"pack {S}", cnt) for cnt in pack_cases().values() for S in (2, 4, 8, 16)]
    for H, row_chunk in ((289, 8), (20, 3)):
        for per_block in (1, 2, 4):
            c = np.random.default_rng(5).integers(0, 1 << 20, -(-13 * -(-H // 8) // per_block))
            cmds.append(command(f"spread 1 100 {H} {per_block} {row_chunk}", c))
    rng = np.random.default_rng(6)
    costs = rng.integers(50, 200, 16 * 9)
    costs[37], costs[90] = 1000, 900
    cmds.append(command("split 128 72 80 4 10", *split_inputs(costs, {37: np.full(64, 50), 90: rng.integers(0, 300, 64)})))
    flat = split_inputs(np.full(16 * 9, 7), {t: np.full(64, 3) for t in range(16 * 9)})
    cmds += [command("split 128 72 100 2 10", *flat), command("split 128 72 0 2 10", *flat),
             command("split 24 24 100 2 10", *split_inputs(np.full(9, 7), {t: np.full(64, 3) for t in range(9)}, 3, 3))]
    return cmds


def test_under_address_and_undefined_sanitizers(planner, tmp):
    """The same program as a stand-alone sanitized binary over the layer-1 inputs: no report
    (either sanitizer ends the program with a failure), and the plain build's words."""
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
    commands = layer1_commands()
    got, want = run_driver(exe, commands), planner(commands)
    assert len(got) == len(want) >= len(commands)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"output {i} differs between the sanitized and the plain build"


# ------------------------------------------------------------------ layer 2

def heavy_tail(rng, n, hi):
    """Mostly small values with many ties, a few large ones."""
    v = rng.integers(0, 8, n) * 10 + (rng.pareto(1.2, n) * 20).astype(np.int64)
    return np.minimum(v, hi)


def golden_cases(seed=GOLDEN_SEED):
    """The seeded inputs of tests/golden/plan_parent.npz, as driver commands, in the fixture's order."""
    rng = np.random.default_rng(seed)
    cmds = [command("by_cost", heavy_tail(rng, 627, 1 << 30))]
    for n in (7, 100):
        cmds += [command(f"shape {mode}", rng.permutation(n)) for mode in (0, 1, 10, 50, 99, 100)]
    for tx, ty, views, block in ((1, 1, 1, 64), (33, 19, 2, 64), (33, 19, 2, 128), (65, 37, 2, 256)):
        cmds.append(command(f"group {tx} {ty} {block}", rng.permutation(-(-tx * ty * views // (block // 64)))))
    for S in (2, 4, 8, 16):
        for ragged in (0, 0, 40):
            cnt = heavy_tail(rng, 64, 65535)
            cnt[rng.permutation(64)[:ragged]] = -1
            cmds.append(command(f"pack {S}", cnt))
    for (W, rows, views), pct, S, mode in (((125, 70, 1), 50, 4, 10), ((125, 70, 2), 25, 8, 0), ((128, 72, 1), 90, 2, 100)):
        tiles = views * -(-W // 8) * -(-rows // 8)
        cmds.append(command(f"split {W} {rows} {pct} {S} {mode}", heavy_tail(rng, views * rows * W, 65535),
                            heavy_tail(rng, tiles, 1 << 30)))
    for H, row_chunk in ((289, 8), (20, 3)):
        for per_block in (1, 2, 4):
            tiles = 2 * 13 * -(-H // 8)
            cmds.append(command(f"spread 2 100 {H} {per_block} {row_chunk}", heavy_tail(rng, -(-tiles // per_block), 1 << 30)))
    return cmds


def test_planners_match_the_parent_word_for_word(planner):
    with np.load(GOLDEN) as z:
        assert int(z["seed"]) == GOLDEN_SEED
        want = [z[f"out{i}"] for i in range(len(z.files) - 1)]
    got = planner(golden_cases())
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w.astype(np.uint32)), f"output {i} differs from the parent's"
