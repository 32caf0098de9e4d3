/* box_comp_emu_driver.cpp -- grid composites through the area-average pass under the fiber emulator: the plan step of
 * ascii-chat_amd/csrc/box.h as box.c runs it, then box_kernel over the plain frames and over the unique tiles and
 * box_canvas_kernel over the composite frames (box_kernels.hpp), launched as box.hip launches them.  TESTS ONLY. */
#include "box_kernels.hpp"

#include <vector>

/* frames[i] (comps[i] != NULL: averaged from that composite) -> images + i * pitch.  counts (may be NULL) receives
 * {unique tiles, plain frames, composite frames, launches issued as bits 0 plain / 1 tiles / 2 canvas}.  Returns 0, or
 * -(refusal) of the first frame the plan step refuses with counts[0..1] = {the frame, the composite source or -1}. */
extern "C" int emu_box_composites(const achip_frame_t *frames, const achip_composite_t *const *comps, int n, uint8_t *images,
                                  uint64_t pitch, int *counts) {
  std::vector<achip_box_desc_t> plain((size_t)n), tiles((size_t)n * 9u);
  std::vector<achip_box_canvas_t> canvas((size_t)n);
  achip_box_plan_t p;
  const int rc = achip_box_plan(frames, comps, n, plain.data(), tiles.data(), canvas.data(), &p);
  if (rc != ACHIP_BOX_OK) {
    if (counts) {
      counts[0] = p.bad_frame;
      counts[1] = p.bad_src;
    }
    return -rc;
  }
  if (pitch < p.image_bytes)
    return -1000;
  int launches = 0;
  const achip_box_uniform_t none = {};
  if (p.n_plain) {
    launches |= 1;
    hipemu::launch(dim3((unsigned)n * (unsigned)p.plain_max_out_h), dim3(ACHIP_BOX_BLOCK), achip::box::lds_bytes(p.plain_max_src_w), [&] {
      achip::box::box_kernel(plain.data(), none, (uint32_t)p.plain_max_out_h, images, pitch);
    });
  }
  /* the scratch slab between guard bytes: a tile stored outside its slot would show */
  const size_t slab_bytes = (size_t)p.n_tiles * (size_t)p.tile_pitch;
  std::vector<uint8_t> slab(slab_bytes + 128u, 0x5A);
  if (p.n_tiles) {
    launches |= 2;
    hipemu::launch(dim3((unsigned)p.n_tiles * (unsigned)p.tile_max_out_h), dim3(ACHIP_BOX_BLOCK), achip::box::lds_bytes(p.tile_max_src_w), [&] {
      achip::box::box_kernel(tiles.data(), none, (uint32_t)p.tile_max_out_h, slab.data() + 64, p.tile_pitch);
    });
    for (size_t i = 0; i < 64u; i++)
      if (slab[i] != 0x5A || slab[64u + slab_bytes + i] != 0x5A)
        return -1001;
  }
  if (p.n_canvas) {
    launches |= 4;
    const uint8_t *tile_base = p.n_tiles ? slab.data() + 64 : nullptr;
    hipemu::launch(dim3((unsigned)p.n_canvas * (unsigned)p.canvas_max_out_h), dim3(ACHIP_BOX_BLOCK), achip::box::lds_bytes(p.canvas_max_w), [&] {
      achip::box::box_canvas_kernel(canvas.data(), (uint32_t)p.canvas_max_out_h, tile_base, p.tile_pitch, images, pitch);
    });
  }
  if (counts) {
    counts[0] = p.n_tiles;
    counts[1] = p.n_plain;
    counts[2] = p.n_canvas;
    counts[3] = launches;
  }
  return 0;
}
