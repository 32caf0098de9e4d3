/*
 * asciichat_raster.h -- libasciichat_raster.so: rendered ANSI frames rasterised to RGBA pixels -- or straight to YUV 4:2:0
 * planes, at the end of this file -- on the device, one font-cell rectangle per character, with a caller-supplied glyph
 * atlas.  The step the reference takes in term_renderer_feed (lib/media/render/terminal.c:405-529, blit_glyph :170-193)
 * before it encodes video.  An opt-in batch pass and NOT a parity path where DESIGN.md 7 says so: every frame starts from a
 * default pen on a blank screen, nothing wraps or scrolls, every codepoint takes one column, and only the grammar below is
 * interpreted.
 *
 * A library of its own: it needs nothing of libasciichat_hip.so and shares only achip_types.h (ACHIP_LEN_OVERFLOW) and the
 * values of the error codes with it.
 *
 * Frame grammar (what this project's renderers, the rain pass and ascii_create_grid emit):
 *   "\n", "\r\n"   column 0 of the next row;  a bare "\r": column 0
 *   UTF-8          one codepoint = one cell, one column; a malformed sequence is U+FFFD and sets BAD_UTF8
 *   ESC [ P.. I.. F  (P 0x30-0x3F, I 0x20-0x2F, F 0x40-0x7E) is one unit:
 *     F == 'm' (SGR), parameters left to right: empty | 0 reset; 38;2;r;g;b / 48;2;r;g;b; 38;5;n / 48;5;n; 30-37, 90-97 indexed
 *       fg 0-15; 40-47, 100-107 indexed bg; 39 / 49 default fg / bg; anything else is ignored and sets UNKNOWN
 *     F == 'b' (REP): the last character written in this row n more times with the current pen (empty n = 1); at a row
 *       start nothing, and UNKNOWN
 *     any other F, other C0 bytes, an ESC without '[': ignored, UNKNOWN
 *   a character at column >= cols is dropped (OVERFLOW_COLS), at row >= rows dropped (OVERFLOW_ROWS)
 * The pen persists across the rows of a frame, not across frames.
 *
 * Compositing (terminal.c:468-525): cells in row-major order; each fills its rectangle with its background, alpha 255, then
 * blits its glyph clipped to the image only -- every pixel of the bitmap rectangle becomes (f*a + b*(255-a)) / 255 per channel
 * of the glyph's own cell's colours, those with a == 0 included.  A pixel therefore shows its last writer in that order.
 */
#ifndef ASCIICHAT_RASTER_H
#define ASCIICHAT_RASTER_H

#include <stddef.h>
#include <stdint.h>

#include "achip_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the values of asciichat_hip.h's codes of the same names */
enum {
  ASCIICHAT_RASTER_OK = 0,
  ASCIICHAT_RASTER_ERR_MEMORY = 3,
  ASCIICHAT_RASTER_ERR_INVALID_PARAM = 86,
  ASCIICHAT_RASTER_ERR_NO_DEVICE = 200 /* no HIP device, or a HIP runtime failure */
};

/* status_dev[i]: the OR of these; 0 = a frame the grammar covers fully */
#define ASCIICHAT_RASTER_NO_FRAME 1u      /* len_dev[i] was ACHIP_LEN_OVERFLOW (or beyond frame_stride): a blank image */
#define ASCIICHAT_RASTER_BAD_UTF8 2u
#define ASCIICHAT_RASTER_UNKNOWN 4u
#define ASCIICHAT_RASTER_OVERFLOW_COLS 8u
#define ASCIICHAT_RASTER_OVERFLOW_ROWS 16u

#define ASCIICHAT_RASTER_INDEXED_FLAT 1  /* every indexed colour is flat_fg / flat_bg (the reference, terminal.c:474-488) */
#define ASCIICHAT_RASTER_INDEXED_XTERM 2 /* 0-15 get_16color_rgb, 16-231 the 0,95,135,175,215,255 cube, 232-255 8 + 10 k */

#define ASCIICHAT_RASTER_MAX_COLS 1024
#define ASCIICHAT_RASTER_MAX_ROWS 512
#define ASCIICHAT_RASTER_MAX_FRAMES 4096
#define ASCIICHAT_RASTER_MAX_GLYPHS 1024
#define ASCIICHAT_RASTER_MAX_COVERAGE (1u << 20)
#define ASCIICHAT_RASTER_MAX_CELL_W 32
#define ASCIICHAT_RASTER_MAX_CELL_H 64

/* One glyph: FreeType's bitmap_left / bitmap_top / bitmap.width / .rows / .pitch, its 8-bit coverage at coverage + offset.
 * Relative to its cell's origin the bitmap covers x0 = left, y0 = baseline - top, x1 = x0 + width, y1 = y0 + rows, which must
 * lie within [-cell_w, 2 cell_w] x [-cell_h, 2 cell_h]; pitch >= width; offset + pitch * rows <= coverage_bytes. */
typedef struct {
  uint32_t codepoint;
  int16_t left, top;
  uint16_t width, rows;
  uint32_t pitch, offset;
} asciichat_raster_glyph_t;

typedef struct {
  int32_t cell_w, cell_h, baseline;       /* 1..32, 1..64, 0..cell_h */
  int32_t n_glyphs;                       /* 0..1024, codepoints strictly ascending */
  const asciichat_raster_glyph_t *glyphs; /* host */
  const uint8_t *coverage;                /* host, 8-bit alpha */
  size_t coverage_bytes;                  /* <= 1 MB */
  uint32_t default_fg, default_bg;        /* 0x00RRGGBB */
  int32_t indexed;                        /* ASCIICHAT_RASTER_INDEXED_FLAT | _XTERM, no default */
  uint32_t flat_fg, flat_bg;              /* FLAT: every indexed colour (reference: 204,204,204 / theme 0 or 255) */
  int32_t matrix_map;                     /* apply matrix_char_map (terminal.c:146-165) before the atlas lookup */
} asciichat_raster_font_t;

typedef struct asciichat_raster asciichat_raster_t;

/* Number of HIP devices (0 when there is none or the runtime fails). */
int asciichat_raster_device_count(void);
/* Message of the calling thread's last failed call ("" when none). */
const char *asciichat_raster_last_error(void);

/* A rasteriser of cols x rows cell frames (1..1024 x 1..512), up to max_frames (1..4096) per run, on the current device.
 * Everything is validated before a device is needed (ERR_INVALID_PARAM), then ERR_NO_DEVICE without one.  The atlas is copied
 * to the device; all scratch of run() is allocated here. */
int asciichat_raster_create(asciichat_raster_t **r, const asciichat_raster_font_t *font, int cols, int rows, int max_frames);
int asciichat_raster_width_px(const asciichat_raster_t *r);     /* cols * cell_w */
int asciichat_raster_height_px(const asciichat_raster_t *r);    /* rows * cell_h */
size_t asciichat_raster_image_pitch(const asciichat_raster_t *r); /* 4 * width * height: bytes of one image, rows tight */

/* Frames as asciichat_hip_plan_render leaves them: frame i at frames_dev + i * frame_stride (< 2^31), len_dev[i] bytes.  Image i goes to
 * pixels_dev + i * image_pitch (4-byte aligned both, image_pitch >= the image's bytes): R, G, B, 255 per pixel, rows 4 * width
 * bytes apart; nothing else is written.  status_dev[i]: the flags above.  1 <= n <= max_frames.  Asynchronous on `stream`:
 * never synchronises, allocates nothing. */
int asciichat_raster_run(asciichat_raster_t *r, const uint8_t *frames_dev, size_t frame_stride, const uint32_t *len_dev, int n,
                         uint8_t *pixels_dev, size_t image_pitch, uint32_t *status_dev, void *stream);
/* run()'s two stages on their own (timing): parse fills the handle's cell grids, raster draws them. */
int asciichat_raster_parse(asciichat_raster_t *r, const uint8_t *frames_dev, size_t frame_stride, const uint32_t *len_dev, int n,
                           uint32_t *status_dev, void *stream);
int asciichat_raster_draw(asciichat_raster_t *r, int n, uint8_t *pixels_dev, size_t image_pitch, void *stream);

/* ---- straight to YUV 4:2:0 planes, for an encoder -------------------------------------------------------------------------
 * The same frames, the same parse and the same compositing, but what is stored is the composited pixel's R, G, B (alpha plays
 * no part) converted by the integer arithmetic of the reference's h265_encoder_ascii_to_yuv420 (lib/video/h265/encoder.c:
 * 247-289), byte for byte:
 *   Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16                         per pixel                               (:264)
 *   r, g, b = (p00 + p10 + p01 + p11) / 4, truncating                   per 2x2 block and channel               (:276-278)
 *   U = ((-38 r - 74 g + 112 b + 128) >> 8) + 128,  V = ((112 r - 94 g - 18 b + 128) >> 8) + 128    (arithmetic shift; :281, :285)
 * (Y is within 16..235 and U, V within 16..240 for every input, so the reference's clamp never acts.)  No RGBA image is
 * written on the way: 1.5 bytes per pixel instead of 4.
 *   I420: Y[W * H], then U[(W/2) * (H/2)], then V[(W/2) * (H/2)], rows tight (W, W/2, W/2) -- encoder.c:248-250, 314-319
 *   NV12: Y[W * H], then (W/2) * (H/2) pairs U, V, rows of W bytes -- what hardware encoders take
 * W = cols * cell_w and H = rows * cell_h must both be even: the reference's loop reads past an odd image and leaves its
 * planes short, which is not reproduced -- the YUV entries refuse such a handle (ERR_INVALID_PARAM, nothing launched). */
#define ASCIICHAT_RASTER_YUV_I420 1
#define ASCIICHAT_RASTER_YUV_NV12 2

size_t asciichat_raster_yuv420_bytes(int width_px, int height_px); /* W * H * 3 / 2; 0 when either is < 2 or odd.  Needs no device */
size_t asciichat_raster_yuv420_pitch(const asciichat_raster_t *r); /* that, of the handle; 0 for NULL or an odd size */
/* As run() and draw(): image i goes to yuv_dev + i * image_pitch (multiples of 4 both, image_pitch >= yuv420_pitch), in
 * `layout`; nothing outside the W * H * 3 / 2 bytes of an image is written; a NO_FRAME frame is the blank image's conversion;
 * status_dev is what run() reports for the same frames.  1 <= n <= max_frames.  Asynchronous on `stream`: never synchronises,
 * allocates nothing.  draw_yuv420 draws the cells the last parse() left. */
int asciichat_raster_run_yuv420(asciichat_raster_t *r, const uint8_t *frames_dev, size_t frame_stride, const uint32_t *len_dev, int n,
                                uint8_t *yuv_dev, size_t image_pitch, int layout, uint32_t *status_dev, void *stream);
int asciichat_raster_draw_yuv420(asciichat_raster_t *r, int n, uint8_t *yuv_dev, size_t image_pitch, int layout, void *stream);

/* ---- straight from the source images, without the text --------------------------------------------------------------------
 * For frames this project's own renderers would write (asciichat_hip_plan_render of the same descriptors, asciichat_hip.h)
 * the text is a detour: what parse() recovers from it -- a glyph, a foreground and a background per cell -- is a function of
 * the pixels the descriptor samples.  These entries fill the handle's cell grids from the descriptors themselves, by the
 * renderers' own sampling, luminance, palette and colour rules; draw() and draw_yuv420() take the cells from there.  Images
 * and status are byte for byte those of plan_render followed by run() / run_yuv420() for the same descriptors, mode and
 * palette.  The cell grids are the handle's, shared with parse(): a draw shows the cells of whichever stage ran last.
 *
 * images_set is the set-up call: mode is ACHIP_MODE_* 0..8 (achip_types.h), palette_chars the renderers' palette, frames a
 * HOST array of n descriptors (1 <= n <= max_frames) whose src are device-visible.  Everything is checked on the host before
 * anything is copied or launched; ERR_INVALID_PARAM, with the handle's earlier set still in place, for
 *   - a mode outside 0..8: ACHIP_MODE_16_DITHER_BG (mode 9), whose cells depend on the error diffused from every cell before
 *     them, is refused here and by images_set_composites and goes through images_set_dithered below;
 *   - a NULL or empty palette, one that is not well-formed UTF-8, or one with a C0 byte or DEL (the grammar reads those as
 *     controls, not as cells);
 *   - n outside 1..max_frames; a descriptor with comp != NULL (those go through images_set_composites) or src == NULL; a size below
 *     1 or a negative padding; (out_w - 1) * x_ratio or (out_h - 1) * y_ratio at 2^32 or above; a source spanning 4 GiB or
 *     more; ops with a dither bit, or with both ACHIP_OP_TINT and ACHIP_OP_FG_OVERRIDE.
 * The descriptors and the mode's glyph table go to the device through a pinned copy the handle owns, asynchronously on
 * `stream`: the caller's array may be freed on return.  The first set of a handle allocates (sized by max_frames), later
 * sets allocate nothing; a set waits on `stream` first when the copy of the set before it may still be in flight.  All calls
 * on one handle must be ordered on ONE stream, sets included, as a plan's are.
 *
 * cells_from_images is the new stage alone, as parse() is: frames 0..n-1 of the last set (1 <= n <= the number set) become
 * cells, status_dev[i] their flags -- only OVERFLOW_COLS (pad_left + out_w beyond cols, in a text row of the grid) and
 * OVERFLOW_ROWS (pad_top + text rows beyond rows) can occur; cells beyond the grid are dropped.  run_images is
 * cells_from_images + draw, run_images_yuv420 is cells_from_images + draw_yuv420; they take and check the output arguments of
 * run() and run_yuv420(), and launch nothing unless every stage takes its arguments.  ERR_INVALID_PARAM before any
 * images_set.  Asynchronous on `stream`: never synchronise, allocate nothing. */
int asciichat_raster_images_set(asciichat_raster_t *r, int mode, const char *palette_chars, const achip_frame_t *frames, int n,
                                void *stream);
/* images_set for the view a server shows every client of a call: the same arguments, lifetime and stream rules, but a frame may
 * carry comp -- a DEVICE-visible achip_composite_t exactly as a plan takes it, from asciichat_hip_composite_upload or from
 * asciichat_hip_grid_composite_dev() (asciichat_hip.h); the grid pokes its source pointers on the device per tick, so one set
 * serves every tick.  A set made by either entry replaces the last one, and cells_from_images, run_images and
 * run_images_yuv420 run whichever is current.  For a composite frame src is not read, src_w x src_h is the canvas the ratios
 * were made for (achip_frame_setup over the W x 2H canvas), flips and tints are ignored and FG_OVERRIDE acts, as in the
 * renderers; pixels outside every tile are black.  Plain and composite frames mix in one set, as in a plan.  The checks are
 * images_set's, except that comp is taken, a frame needs src or comp, and a composite frame has no source extent to check; every
 * set taken here is one asciichat_hip_plan_create takes, and cells, images and status are byte for byte those of plan_render
 * followed by run() / run_yuv420().  A set without a composite frame costs what images_set's does.
 * The descriptor is read by the staged sampler the renderers use: its _pad word must be zero (it is the pixel of every sample
 * outside the tiles) and a grid without cells (cell_w, cell_h, cols or rows of 0) must have n_src == 0.  composite_upload
 * guarantees both; a descriptor placed on the device by other means must keep them. */
int asciichat_raster_images_set_composites(asciichat_raster_t *r, int mode, const char *palette_chars, const achip_frame_t *frames, int n,
                                           void *stream);
/* images_set for the Floyd-Steinberg renderer, ACHIP_MODE_16_DITHER_BG -- what a truecolor client in the background render mode
 * is shown (achip_mode_from_caps).  The mode is implied; images_set and images_set_composites keep refusing mode 9 and every
 * dither bit in ops, and this entry takes them.  Arguments, lifetime, stream, pinned-copy and allocation rules are those of the
 * other two set calls; a set made by any of the three replaces the last one, and cells_from_images, run_images and
 * run_images_yuv420 run whichever is current, their arguments and checks unchanged.  A frame may be plain (src) or a composite
 * (comp, device-visible, as images_set_composites takes it), both kinds in one set; its ops may carry the style bits of
 * achip_frame_set_dither_style, a style per frame: none is the background form, ACHIP_OP_DITHER_FG the foreground-only form
 * with the glyph cache[Y], ACHIP_OP_DITHER_FG | ACHIP_OP_DITHER_RAMP the one with the glyph cache[ramp[Y >> 2]].  Flips and
 * tints act as in the renderer (not on a composite frame); FG_OVERRIDE is taken and changes nothing, for this mode emits no
 * truecolor SGR.  The frame's out_w x out_h samples are dithered on the device in the renderer's order and arithmetic (7/3/5/1
 * sixteenths, each truncated toward zero; what leaves the image is dropped; the clamped value is quantised, the unclamped one
 * gives the error): columns beyond the grid still feed the row below, rows behind the grid are not computed.  Cells, images,
 * YUV planes and status are byte for byte those of asciichat_hip_plan_render of the same descriptors in mode 9 followed by
 * run() / run_yuv420(), for INDEXED_FLAT and INDEXED_XTERM fonts, with and without matrix_map.
 * ERR_INVALID_PARAM, checked on the host before anything is copied or launched and with the earlier set still in place, for
 * everything images_set_composites refuses except dither bits, for ACHIP_OP_DITHER_RAMP without ACHIP_OP_DITHER_FG, and --
 * A BOUND OF THIS ENTRY -- for a frame with out_w > ASCIICHAT_RASTER_MAX_COLS (1024): no handle can show such a row, and the
 * bound sizes the kernel's error line. */
int asciichat_raster_images_set_dithered(asciichat_raster_t *r, const char *palette_chars, const achip_frame_t *frames, int n,
                                         void *stream);
int asciichat_raster_cells_from_images(asciichat_raster_t *r, int n, uint32_t *status_dev, void *stream);
int asciichat_raster_run_images(asciichat_raster_t *r, int n, uint8_t *pixels_dev, size_t image_pitch, uint32_t *status_dev,
                                void *stream);
int asciichat_raster_run_images_yuv420(asciichat_raster_t *r, int n, uint8_t *yuv_dev, size_t image_pitch, int layout,
                                       uint32_t *status_dev, void *stream);

void asciichat_raster_destroy(asciichat_raster_t *r);

#ifdef __cplusplus
}
#endif
#endif
