// oracle/ref_trace.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the reference's own tracers and tree edits, compiled where they lie
// (no copies, no stand-ins for any arithmetic):
//   och::h_octree<19, D>::set / sse_trace / get_root   ORT/och_h_octree.h
//   och::octree::set / unset / sse_trace / get_node_cnt ORT/och_octree.cpp
// Built by oracle/Makefile into oracle/_ref/ (git-ignored) with
// oracle/msvc_shim/intrin.h standing where MSVC's <intrin.h> would.
// och_z_order.cpp and och_octree.cpp are included into this one translation
// unit: z_encode_16 is __forceinline there and is not emitted otherwise.
//
// Protocol (binary, little-endian, stdin -> stdout):
//   ref_trace h <depth>             h_octree<19, depth>
//   ref_trace o <depth> <capacity>  octree(depth, capacity)
//   stdin : u32 n_ops, u32 n_rays,
//           n_ops  x (u32 x, u32 y, u32 z, u32 v)   h: set(x, y, z, v)
//                                                   o: v != 0 set, v == 0 unset
//           n_rays x (f32 ox, oy, oz, dx, dy, dz)
//   stdout: n_rays x (i32 direction, u32 voxel, f32 t), then one u32:
//           h: get_root()   o: get_node_cnt()
// Rays must be finite: the reference need not terminate on NaN or inf.
//
// h_octree's depth is a template argument: 2, 3, 4, 6, 8, 10, 12 and 16 are
// instantiated (set() packs coordinates with z_encode_16 and stops at 16).
// Depth 1 is left out: its parent stack, uint32_t parents[depth - 1], would
// have length zero.  The trees are created with new and never destroyed (the
// reference's destructors delete[] what a plain new allocated); the process
// flushes stdout and leaves with _Exit(0).
#include <cstdint>
#include <cstdio>
#include <cmath>      // INFINITY, which MSVC's headers hand och_h_octree.h:429 unasked
#include <cstdlib>
#include <vector>

#include "och_z_order.cpp"
#include "och_octree.cpp"
#include "och_h_octree.h"

namespace
{
    struct op_rec { uint32_t x, y, z, v; };
    struct ray_rec { float ox, oy, oz, dx, dy, dz; };
    struct hit_rec { int32_t direction; uint32_t voxel; float t; };

    std::vector<op_rec> ops;
    std::vector<ray_rec> rays;

    bool read_input()
    {
        uint32_t head[2];
        if (std::fread(head, sizeof head, 1, stdin) != 1) return false;
        ops.resize(head[0]);
        rays.resize(head[1]);
        if (head[0] && std::fread(ops.data(), sizeof(op_rec), head[0], stdin) != head[0]) return false;
        if (head[1] && std::fread(rays.data(), sizeof(ray_rec), head[1], stdin) != head[1]) return false;
        return true;
    }

    template<typename Tree>
    void trace_all(const Tree& tree, uint32_t tail)
    {
        std::vector<hit_rec> out(rays.size());
        for (size_t i = 0; i != rays.size(); ++i)
        {
            const ray_rec& r = rays[i];
            och::direction dir = och::direction::error;
            uint32_t voxel = 0;
            float t = 0.0F;
            tree.sse_trace(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, dir, voxel, t);
            out[i].direction = static_cast<int32_t>(dir);
            out[i].voxel = voxel;
            out[i].t = t;
        }
        if (!out.empty()) std::fwrite(out.data(), sizeof(hit_rec), out.size(), stdout);
        std::fwrite(&tail, 4, 1, stdout);
    }

    template<int Depth>
    void run_h()
    {
        auto* tree = new och::h_octree<19, Depth>;
        for (const op_rec& o : ops)
            tree->set(static_cast<uint16_t>(o.x), static_cast<uint16_t>(o.y), static_cast<uint16_t>(o.z), o.v);
        trace_all(*tree, tree->get_root());
    }

    void run_o(int depth, uint32_t capacity)
    {
        auto* tree = new och::octree(static_cast<uint16_t>(depth), capacity);
        for (const op_rec& o : ops)
            if (o.v)
                tree->set(static_cast<int16_t>(o.x), static_cast<int16_t>(o.y), static_cast<int16_t>(o.z), o.v);
            else
                tree->unset(static_cast<int16_t>(o.x), static_cast<int16_t>(o.y), static_cast<int16_t>(o.z));
        trace_all(*tree, static_cast<uint32_t>(tree->get_node_cnt()));
    }

    [[noreturn]] void leave(int code)
    {
        std::fflush(stdout);
        std::_Exit(code);
    }
}

int main(int argc, char** argv)
{
    if (argc < 3 || (argv[1][0] != 'h' && argv[1][0] != 'o') || argv[1][1])
    {
        std::fprintf(stderr, "usage: ref_trace h <depth> | o <depth> <capacity>\n");
        return 2;
    }
    const int depth = std::atoi(argv[2]);
    if (!read_input())
    {
        std::fprintf(stderr, "ref_trace: short input\n");
        return 3;
    }
    if (argv[1][0] == 'h')
    {
        const uint32_t dim = 1u << depth;
        for (const op_rec& o : ops)
            if ((o.x | o.y | o.z) >= 65536u || depth > 16 || (o.x | o.y | o.z) >= dim)
            {
                std::fprintf(stderr, "ref_trace: voxel outside the tree\n");
                return 3;
            }
        switch (depth)
        {
        case 2: run_h<2>(); break;
        case 3: run_h<3>(); break;
        case 4: run_h<4>(); break;
        case 6: run_h<6>(); break;
        case 8: run_h<8>(); break;
        case 10: run_h<10>(); break;
        case 12: run_h<12>(); break;
        case 16: run_h<16>(); break;
        default:
            std::fprintf(stderr, "ref_trace: h_octree depth %d is not instantiated\n", depth);
            return 2;
        }
    }
    else
    {
        // octree::sse_trace keeps 13 parents and unset() a 13-entry stack;
        // int16_t coordinates: depth 2 .. 14.
        if (argc < 4 || depth < 2 || depth > 14)
        {
            std::fprintf(stderr, "ref_trace: octree needs depth 2 .. 14 and a capacity\n");
            return 2;
        }
        const uint32_t capacity = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10));
        const uint32_t dim = 1u << depth;
        if (capacity < 2) return 2;
        for (const op_rec& o : ops)
            if ((o.x | o.y | o.z) >= dim)
            {
                std::fprintf(stderr, "ref_trace: voxel outside the tree\n");
                return 3;
            }
        run_o(depth, capacity);
    }
    leave(0);
}
