// examples/render_frame.cpp -- headless C++ host over the C ABI: builds the
// demo terrain, renders one frame on the GPU into an RGBA8 buffer (the
// olc::Pixel layout the reference's window blits) and writes it as a PPM.
// Also traces the reference's per-frame pick ray (ORT/test_och_h_octree.cpp:527-536)
// through the reference signature, tree.sse_trace(o, d, dir&, voxel&, t&).
//
//   make -C examples && ./examples/render_frame 10 out.ppm [width height yaw pitch] [--ssaa S] [--lit]
//
// --ssaa S (2, 4 or 8, anywhere on the line): the same width x height frame
// from S x S samples per pixel, resolved in the render kernel (tree.render_ssaa).
// --lit (anywhere on the line): the frame with sun shadows and ambient
// occlusion, secondary rays traced in the render's launch (tree.render_lit).
// Both flags, in either order: S x S lit samples per pixel, shaded and then
// averaged in one launch (tree.render_lit_ssaa).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "och_gpu.hpp"
#include "palette.hpp"

int main(int argc, char **argv)
{
    int ssaa = 0;
    bool lit = false;
    for (int i = 1; i < argc; ++i)
        if (std::strcmp(argv[i], "--lit") == 0) {       // taken out of the positional arguments
            lit = true;
            for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
            argc -= 1;
            break;
        }
    for (int i = 1; i + 1 < argc; ++i)
        if (std::strcmp(argv[i], "--ssaa") == 0) {      // taken out of the positional arguments
            ssaa = std::atoi(argv[i + 1]);
            for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    const int depth = argc > 1 ? std::atoi(argv[1]) : 10;
    const char *path = argc > 2 ? argv[2] : "frame.ppm";
    och::gpu::camera cam;
    cam.width = argc > 4 ? std::atoi(argv[3]) : 1280;
    cam.height = argc > 4 ? std::atoi(argv[4]) : 720;
    cam.yaw = argc > 6 ? std::strtof(argv[5], nullptr) : 0.3F;
    cam.pitch = argc > 6 ? std::strtof(argv[6], nullptr) : -0.6F;
    och_terrain_params tp = {depth, 1, 1, 0, 0, 1};   // voxelised on the GPU
    och_host_pool hp;
    och::gpu::check(och_build_terrain(&tp, &hp), "och_build_terrain");
    std::printf("terrain depth %d: %u nodes (%.2f s)\n", depth, hp.n_nodes, hp.build_seconds);
    try {
        och::gpu::tree tree(hp.nodes, hp.n_nodes, hp.root, hp.depth);
        tree.set_palette(examples::reference_palette());
        std::vector<uint32_t> rgba((size_t)cam.width * cam.height);
        // the sun over the camera's left shoulder; AO rays reach eight voxels along each axis
        const och_light light = {{0.8F, 0.35F, 0.25F}, std::ldexp(8.0F, -depth), 96, 24, OCH_LIGHT_SUN | OCH_LIGHT_AO};
        if (ssaa) {
            och::gpu::camera samples = cam;             // the sample grid's camera
            samples.width *= ssaa;
            samples.height *= ssaa;
            if (lit)
                tree.render_lit_ssaa(samples.update_position(), light, ssaa, rgba);
            else
                tree.render_ssaa(samples.update_position(), ssaa, rgba);
            std::printf("%d x %d samples per pixel\n", ssaa, ssaa);
        } else if (lit) {
            tree.render_lit(cam.update_position(), light, rgba);
        } else {
            tree.render(cam.update_position(), rgba.data());
        }
        if (lit)
            std::printf("lit: sun (%g, %g, %g), ao reach %g\n", light.sun_dir[0], light.sun_dir[1], light.sun_dir[2],
                        light.ao_reach);
        // pick ray along the view direction (the demo traces camera.pos along its look vector)
        const float dx = cosf(cam.yaw) * cosf(cam.pitch), dy = sinf(cam.yaw) * cosf(cam.pitch), dz = sinf(cam.pitch);
        och::gpu::direction dir;
        uint32_t vox;
        float t;
        tree.sse_trace(cam.pos, {dx, dy, dz}, dir, vox, t);
        std::printf("pick ray: d %a %a %a direction %d voxel %u t %a\n", dx, dy, dz, (int)dir, vox, t);
        if (!examples::write_ppm(path, rgba.data(), cam.width, cam.height)) return 1;
        std::printf("wrote %s\n", path);
    } catch (const och::gpu::error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        och_host_pool_free(&hp);
        return 1;
    }
    och_host_pool_free(&hp);
    return 0;
}
