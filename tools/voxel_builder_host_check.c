/* Stand-alone host check of och_build_voxels (use_gpu = 0): small lists and a
 * grid, each built and read back voxel by voxel with och_pool_at against a
 * last-wins replay of the records; then och_build_terrain's host path at depths
 * 6 and 7.  Meant to be linked against the builders' host code (csrc/och_builder.cpp
 * with och_dag.h and och_voxel_build.h) compiled with AddressSanitizer +
 * UndefinedBehaviorSanitizer (tools/voxel_builder_sanitize.sh); needs no GPU.
 * Exit status 0 = all equal. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "och_gpu.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            fprintf(stderr, __VA_ARGS__); \
            fputc('\n', stderr);          \
            ++failures;                   \
        }                                 \
    } while (0)

/* What successive set() calls leave at record i's coordinate: the id of the last record there. */
static uint32_t last_at(const uint32_t *rec, uint64_t n, uint32_t x, uint32_t y, uint32_t z)
{
    uint32_t id = 0;
    for (uint64_t i = 0; i < n; ++i)
        if (rec[4 * i] == x && rec[4 * i + 1] == y && rec[4 * i + 2] == z) id = rec[4 * i + 3];
    return id;
}

static void check_list(const char *name, int depth, const uint32_t *rec, uint64_t n, int threads)
{
    och_voxel_params p;
    och_host_pool pool;
    memset(&p, 0, sizeof p);
    p.depth = depth;
    p.kind = OCH_VOXELS_LIST;
    p.data = rec;
    p.n = n;
    p.threads = threads;
    const int st = och_build_voxels(&p, &pool);
    CHECK(st == OCH_OK, "%s: status %d (%s)", name, st, och_last_error());
    if (st != OCH_OK) return;
    const uint32_t dim = 1u << depth;
    uint64_t solid = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t x = rec[4 * i], y = rec[4 * i + 1], z = rec[4 * i + 2];
        if (x >= dim || y >= dim || z >= dim) continue;
        const uint32_t want = last_at(rec, n, x, y, z);
        const uint32_t got = och_pool_at(pool.nodes, pool.root, depth, 1, (int)x, (int)y, (int)z);
        CHECK(got == want, "%s: (%u, %u, %u) holds %u, expected %u", name, x, y, z, got, want);
        /* count a coordinate once, at its last record */
        int last = 1;
        for (uint64_t j = i + 1; j < n && last; ++j)
            last = !(rec[4 * j] == x && rec[4 * j + 1] == y && rec[4 * j + 2] == z);
        solid += last && want != 0;
    }
    CHECK(pool.solid_voxels == solid, "%s: %llu solid voxels, expected %llu", name, (unsigned long long)pool.solid_voxels,
          (unsigned long long)solid);
    CHECK((pool.root != 0) == (solid != 0) && pool.n_nodes >= 1, "%s: root %u of %u nodes", name, pool.root, pool.n_nodes);
    och_host_pool_free(&pool);
}

static uint32_t *random_list(uint64_t n, int depth, int spread)
{
    uint32_t *rec = malloc((n ? n : 1) * 16);
    for (uint64_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) rec[4 * i + k] = rnd() % ((1u << depth) + (uint32_t)spread);
        rec[4 * i + 3] = rnd() % 5 ? rnd() : 0; /* any uint32 id; a fifth are removals */
        if (i > 4 && rnd() % 4 == 0) memcpy(rec + 4 * i, rec + 4 * (rnd() % i), 12); /* a quarter repeat a coordinate */
    }
    return rec;
}

int main(void)
{
    static const uint64_t sizes[] = {0, 1, 8, 63, 64, 65, 257, 3000};
    static const int depths[] = {1, 3, 7, 16, 21};
    char name[64];
    for (size_t s = 0; s < sizeof sizes / sizeof *sizes; ++s)
        for (size_t d = 0; d < sizeof depths / sizeof *depths; ++d) {
            /* small trees get records outside them as well */
            uint32_t *rec = random_list(sizes[s], depths[d] > 3 ? 3 : depths[d], depths[d] <= 3 ? 2 : 0);
            if (depths[d] > 3) /* deep trees: a cluster at each end of the cube */
                for (uint64_t i = 0; i < sizes[s]; i += 2)
                    for (int k = 0; k < 3; ++k) rec[4 * i + k] = (1u << depths[d]) - 1 - rec[4 * i + k];
            snprintf(name, sizeof name, "list n=%llu depth=%d", (unsigned long long)sizes[s], depths[d]);
            check_list(name, depths[d], rec, sizes[s], 1 + (int)(s % 3));
            free(rec);
        }

    /* a grid and a caller's capacity */
    uint8_t grid[8 * 8 * 8];
    for (size_t i = 0; i < sizeof grid; ++i) grid[i] = rnd() % 3 ? 0 : (uint8_t)(1 + rnd() % 200);
    och_voxel_params p;
    och_host_pool pool;
    memset(&p, 0, sizeof p);
    p.depth = 3;
    p.kind = OCH_VOXELS_GRID_U8;
    p.data = grid;
    CHECK(och_build_voxels(&p, &pool) == OCH_OK, "grid: %s", och_last_error());
    for (int z = 0; z < 8; ++z)
        for (int y = 0; y < 8; ++y)
            for (int x = 0; x < 8; ++x)
                CHECK(och_pool_at(pool.nodes, pool.root, 3, 1, x, y, z) == grid[(z * 8 + y) * 8 + x], "grid: (%d, %d, %d)", x, y, z);
    och_host_pool_free(&pool);

    const uint32_t one[4] = {5, 6, 7, 1};
    memset(&p, 0, sizeof p);
    p.depth = 9;
    p.kind = OCH_VOXELS_LIST;
    p.data = one;
    p.n = 1;
    p.capacity = 9;
    CHECK(och_build_voxels(&p, &pool) == OCH_E_CAPACITY, "capacity 9 of 10 was accepted");
    p.capacity = 10;
    CHECK(och_build_voxels(&p, &pool) == OCH_OK && pool.n_nodes == 9, "capacity 10 of 10 was refused");
    och_host_pool_free(&pool);
    p.depth = 22;
    CHECK(och_build_voxels(&p, &pool) == OCH_E_INVALID, "depth 22 was accepted");

    /* the host terrain builder: one and two levels above the 32^3 bricks (reduce_grid
     * over the brick roots) and the leaf-code map, as a DAG and as an expanded tree;
     * the pool does not depend on the thread count, and the expanded tree has
     * exactly the nodes the DAG build counted */
    for (int depth = 6; depth <= 7; ++depth) {
        uint64_t tree_nodes = 0;
        for (int dedup = 1; dedup >= 0; --dedup) {
            och_host_pool built[2];
            static const int thread_counts[2] = {1, 3};
            int ok = 1;
            for (int t = 0; t < 2; ++t) {
                och_terrain_params tp;
                memset(&tp, 0, sizeof tp);
                tp.depth = depth;
                tp.tunnels = 1;
                tp.dedup = dedup;
                tp.threads = thread_counts[t];
                const int st = och_build_terrain(&tp, &built[t]);
                CHECK(st == OCH_OK, "terrain depth %d dedup %d threads %d: status %d (%s)", depth, dedup, tp.threads, st,
                      och_last_error());
                if (st != OCH_OK) built[t].nodes = NULL;
                ok = ok && st == OCH_OK;
            }
            if (ok) {
                CHECK(built[0].n_nodes == built[1].n_nodes && built[0].root == built[1].root &&
                          !memcmp(built[0].nodes, built[1].nodes, (size_t)built[0].n_nodes * 32),
                      "terrain depth %d dedup %d: 1 and 3 threads differ (%u, %u nodes)", depth, dedup, built[0].n_nodes,
                      built[1].n_nodes);
                CHECK(built[0].tree_nodes == built[1].tree_nodes && built[0].solid_voxels == built[1].solid_voxels,
                      "terrain depth %d dedup %d: statistics differ between 1 and 3 threads", depth, dedup);
                if (dedup) tree_nodes = built[0].tree_nodes;
                else
                    CHECK(built[0].n_nodes == tree_nodes && built[0].tree_nodes == tree_nodes,
                          "terrain depth %d: the expanded tree has %u nodes, tree_nodes %llu / %llu", depth, built[0].n_nodes,
                          (unsigned long long)built[0].tree_nodes, (unsigned long long)tree_nodes);
            }
            for (int t = 0; t < 2; ++t) och_host_pool_free(&built[t]);
        }
    }

    printf(failures ? "voxel_builder_host_check: %d failures\n" : "voxel_builder_host_check: ok\n", failures);
    return failures != 0;
}
