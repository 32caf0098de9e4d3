/*
 * zpack.c -- the wire stage with the frames compressed on the device (asciichat_hip_frame_packets_zpacked): checksums,
 * headers and the frames in pack_frames' layout over the lengths AS SENT, every frame either as it is or as a "zhuf" zstd
 * frame (raw, RLE and Huffman-literals blocks, zero sequences: zpack_kernels.hpp) by the reference sender's own
 * rule.  Asynchronous: four launches on the caller's stream, the scratch is the caller's.  No plan and no drop-in entry takes
 * this form by itself.  The _wide entries are the same pass over all 256 byte values (the tree in zstd's FSE-compressed form
 * where a piece holds a byte above 0x80), with a larger scratch record; they are as opt-in as the narrow ones.  The _seq entries
 * are the sequence form (zseq_kernels.hpp): blocks of 8 KB, matches of a 64-byte window as zstd sequences under the predefined
 * tables, the other bytes as the wide form's literals; opt-in likewise, with a scratch of its own layout.
 */
#include <stdint.h>

#include "asciichat_hip.h"
#include "internal.h"
#include "zpack.h"

/* the three forms: what differs between them on the host side.  `entry` names the frame_packets entry in messages. */
enum { FORM_NARROW = 0, FORM_WIDE = 1, FORM_SEQ = 2 };
static const struct zpack_form {
  const char *entry;
  uint32_t (*pieces)(uint32_t max_len);
  size_t (*scratch_bytes)(uint32_t max_len, int n);
  achip_zpack_launch_fn *launch;
  const char *launch_label;
} FORMS[] = {
    [FORM_NARROW] = {"frame_packets_zpacked", achip_zpack_pieces, achip_zpack_scratch_bytes, achip_launch_zpack, "zpack launch"},
    [FORM_WIDE] = {"frame_packets_zpacked_wide", achip_zpack_pieces, achip_zpack_wide_scratch_bytes, achip_launch_zpack_wide, "zpack wide launch"},
    [FORM_SEQ] = {"frame_packets_zpacked_seq", achip_zseq_pieces, achip_zseq_scratch_bytes, achip_launch_zseq, "zseq launch"},
};

static size_t form_scratch_bytes(int form, uint32_t max_len, int n) {
  if (max_len == 0 || max_len >= 0xFFFFFFF0u)
    return 0;
  return FORMS[form].scratch_bytes(max_len, n);
}

static int frame_packets_zpacked(int form, const uint8_t *base_dev, size_t stride, const uint32_t *len_dev, uint32_t max_len, int n,
                                 const uint32_t *dims_dev, uint32_t *crc_out_dev, uint8_t *hdr_out_dev, uint32_t *packet_crc_out_dev, uint8_t *dst,
                                 size_t dst_capacity, uint64_t *off_out, uint32_t *len_out, void *scratch_dev, size_t scratch_bytes,
                                 void *stream) {
  const struct zpack_form *f = &FORMS[form];
  const char *what = f->entry;
  if (!base_dev || !crc_out_dev || n <= 0 || ((uintptr_t)base_dev & 15u) || (stride & 15u) || max_len == 0 || max_len >= 0xFFFFFFF0u ||
      (n > 1 && stride < max_len))
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "%s: bad arguments", what);
  if (!len_dev || !hdr_out_dev || !dst || ((uintptr_t)dst & 15u) || ((uintptr_t)off_out & 7u) || ((uintptr_t)len_out & 3u) ||
      ((uintptr_t)hdr_out_dev & 7u))
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "%s: lengths, a header buffer and a 16-byte aligned destination are required", what);
  if ((uint64_t)n * f->pieces(max_len) > 0x7FFFFFFFull)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "%s: %d frames of up to %u bytes are more pieces than a launch takes", what, n, max_len);
  const size_t need = f->scratch_bytes(max_len, n);
  if (!scratch_dev || ((uintptr_t)scratch_dev & 7u) || scratch_bytes < need)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "%s: an 8-byte aligned scratch of %zu bytes is required (%zu given)", what, need,
                      scratch_bytes);
  const int rc = achip_require_device();
  if (rc)
    return rc;
  return achip_hip_check(f->launch(base_dev, (uint64_t)stride, len_dev, max_len, n, dims_dev, crc_out_dev, hdr_out_dev, packet_crc_out_dev, dst,
                                   (uint64_t)dst_capacity, off_out, len_out, (uint32_t *)scratch_dev, stream),
                         f->launch_label);
}

/* plan render + the pass above on one stream.  Always these two steps: the plan's own choices among the packed forms do not
 * apply here, and no plan takes this form by itself. */
static int plan_render_packets_zpacked(int form, asciichat_hip_plan_t *p, uint8_t *slab_dev, size_t out_stride, uint32_t *out_len_dev,
                                       const uint32_t *dims_dev, uint32_t *crc_out_dev, uint8_t *hdr_out_dev, uint32_t *packet_crc_out_dev,
                                       uint8_t *dst, size_t dst_capacity, uint64_t *off_out, uint32_t *len_out, void *scratch_dev,
                                       size_t scratch_bytes, void *stream) {
  const char *what = FORMS[form].entry + sizeof("frame_packets_") - 1; /* "zpacked", "zpacked_wide", "zpacked_seq" */
  if (!p || !hdr_out_dev || !dst || !scratch_dev)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "plan_render_packets_%s: no plan, header buffer, destination or scratch", what);
  if (out_stride == 0 || out_stride >= 0xFFFFFFF0u)
    return achip_fail(ASCIICHAT_HIP_ERR_INVALID_PARAM, "plan_render_packets_%s: stride %zu", what, out_stride);
  int rc = asciichat_hip_plan_render(p, slab_dev, out_stride, out_len_dev, stream);
  if (!rc)
    rc = frame_packets_zpacked(form, slab_dev, out_stride, out_len_dev, (uint32_t)out_stride, achip_plan_frame_count(p), dims_dev, crc_out_dev,
                               hdr_out_dev, packet_crc_out_dev, dst, dst_capacity, off_out, len_out, scratch_dev, scratch_bytes, stream);
  return rc;
}

/* the exported entries of one form: asciichat_hip_zpack<infix>_scratch_bytes, asciichat_hip_frame_packets_zpacked<infix> and
 * asciichat_hip_plan_render_packets_zpacked<infix> (asciichat_hip.h) */
#define ZPACK_ENTRIES(form, infix)                                                                                                      \
  size_t asciichat_hip_zpack##infix##_scratch_bytes(uint32_t max_len, int n) { return form_scratch_bytes(form, max_len, n); }           \
  int asciichat_hip_frame_packets_zpacked##infix(const uint8_t *base_dev, size_t stride, const uint32_t *len_dev, uint32_t max_len,     \
                                                 int n, const uint32_t *dims_dev, uint32_t *crc_out_dev, uint8_t *hdr_out_dev,          \
                                                 uint32_t *packet_crc_out_dev, uint8_t *dst, size_t dst_capacity, uint64_t *off_out,    \
                                                 uint32_t *len_out, void *scratch_dev, size_t scratch_bytes, void *stream) {            \
    return frame_packets_zpacked(form, base_dev, stride, len_dev, max_len, n, dims_dev, crc_out_dev, hdr_out_dev, packet_crc_out_dev,   \
                                 dst, dst_capacity, off_out, len_out, scratch_dev, scratch_bytes, stream);                              \
  }                                                                                                                                     \
  int asciichat_hip_plan_render_packets_zpacked##infix(asciichat_hip_plan_t *p, uint8_t *slab_dev, size_t out_stride,                   \
                                                       uint32_t *out_len_dev, const uint32_t *dims_dev, uint32_t *crc_out_dev,          \
                                                       uint8_t *hdr_out_dev, uint32_t *packet_crc_out_dev, uint8_t *dst,                \
                                                       size_t dst_capacity, uint64_t *off_out, uint32_t *len_out, void *scratch_dev,    \
                                                       size_t scratch_bytes, void *stream) {                                            \
    return plan_render_packets_zpacked(form, p, slab_dev, out_stride, out_len_dev, dims_dev, crc_out_dev, hdr_out_dev,                  \
                                       packet_crc_out_dev, dst, dst_capacity, off_out, len_out, scratch_dev, scratch_bytes, stream);    \
  }

ZPACK_ENTRIES(FORM_NARROW, )
ZPACK_ENTRIES(FORM_WIDE, _wide)
ZPACK_ENTRIES(FORM_SEQ, _seq)
