// och_hash.h -- the hash of a DAG node's key, (height above the voxels, 8 child
// words): the host store's (NodeStore) and the device probe's (probe_node), both
// in och_dag.h; a table slot is its low bits.  Plain C++ and HIP-free, so that a
// host program can include it and state which rows meet in one slot
// (tests/intern_cases.py holds the numpy twin).
#pragma once
#include <stdint.h>

// as och_terrain.h defines it
#ifndef OCH_HD
#if defined(__HIPCC__)
#define OCH_HD __host__ __device__ __forceinline__
#else
#define OCH_HD inline
#endif
#endif

namespace och_hash {

OCH_HD uint64_t mix64(uint64_t h)
{
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return h;
}

// The hash of a node's key, level h and child words c: the host store's and
// the device probe's (a table slot is its low bits).
OCH_HD uint64_t node_hash(const uint32_t c[8], int h)
{
    uint64_t hs = mix64((uint64_t)h * 0x9E3779B97F4A7C15ull ^ ((uint64_t)c[1] << 32 | c[0]));
    hs = mix64(hs ^ ((uint64_t)c[3] << 32 | c[2]));
    hs = mix64(hs ^ ((uint64_t)c[5] << 32 | c[4]));
    hs = mix64(hs ^ ((uint64_t)c[7] << 32 | c[6]));
    return hs;
}

}  // namespace och_hash
