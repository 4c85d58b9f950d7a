/* srk.h -- C ABI of libsrk_gfx950.so: the MI355X (gfx950) kernels for the SR convolutional hot path.
 *
 * The reference (george-gca/sr-pytorch-lightning) has no FFI layer: its hot path is
 * `SRModel.forward()` (models/srmodel.py:156-171) calling stock torch.nn leaf modules
 * (SURVEY.md section 8(b)).  The entry points below are what a binding for that path
 * has to call; each one names the reference op it replaces.  The Python binding that
 * ships with this repo is `sr-pytorch-lightning_amd/_lib.py` (ctypes), and
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - All pointers are DEVICE pointers owned by the caller (torch tensors in practice).
 *    The library allocates nothing persistent and never frees.
 *  - Every launcher takes the HIP stream to enqueue on; it never synchronises and
 *    never touches the null stream, so it can be captured into a hipGraph.
 *  - Return value: 0 on success, otherwise a hipError_t or a negative SRK_E_* code;
 *    `srk_last_error()` returns a thread-local message.  No exceptions cross the ABI.
 *  - Launchers are re-entrant and hold no mutable global state (autograd calls
 *    backward from another thread).  The one exception is write-once and
 *    mutex-guarded: the per-device upload stream of srk_upload_prepare / _eager / _fence.
 *  - Activations are NHWC with an explicit pixel pitch and channel offset (both in
 *    elements) so that a conv can read / write a channel slice of a wider buffer
 *    (RDN dense blocks, models/rdn.py:21).  Channel counts seen by the MFMA kernels are
 *    padded to a multiple of 16 with ZERO-filled padding channels.
 *  - dtype: SRK_BF16 / SRK_F16 storage with fp32 accumulate, or SRK_F32 (fp32 MFMA,
 *    the parity mode: north_star "conv activations within 1e-3 fp32").
 */
#ifndef SRK_H
#define SRK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* srk_stream_t; /* hipStream_t */

enum { SRK_BF16 = 0, SRK_F16 = 1, SRK_F32 = 2 };

enum {
  SRK_E_BADARG = -1,   /* shape / alignment / mode not supported */
  SRK_E_NODEV = -2     /* no gfx950 device / kernel image not loadable */
};

/* output / residual addressing modes of srk_conv2d */
enum {
  SRK_OUT_NHWC = 0,      /* out[n][y][x][coff + co], dtype = args.dtype                               */
  SRK_OUT_NHWC_PS = 1,   /* conv followed by nn.PixelShuffle(r) (models/common.py:133), fused into the  */
                         /* store: out[n][y*r+i][x*r+j][coff + c]; packed channel co' = (i*r+j)*C + c   */
  SRK_OUT_PLANAR = 2     /* fp32 NCHW (the model boundary), optional PixelShuffle(r):                   */
                         /* out[n][c][y*r+i][x*r+j], co = c*r*r + i*r + j (torch channel order)         */
};

/* ---- weight packing -------------------------------------------------------------------------
 * Replaces nothing in the reference: it converts the parameters of record (OIHW fp32, the
 * state_dict layout of nn.Conv2d) into the MFMA-friendly shadow layout
 *     wpk[tap][Kin/CH][CoutP][CH]      CH = 16 bytes / sizeof(dtype)
 * forward : Kin = Cin padded to 16,  rows = Cout padded to CoutP, tap = kh*KW+kw
 * dgrad   : Kin = Cout padded to 16, rows = Cin padded to CoutP, tap flipped (conv transpose)
 * `ps_r` > 1 applies the PixelShuffle channel permutation of SRK_OUT_NHWC_PS to the Cout axis.
 * bias_pk (nullable) receives the fp32 bias padded/permuted to CoutP (forward only).           */
typedef struct {
  const float* w;      /* [Cout][Cin][KH][KW] fp32 */
  const float* bias;   /* [Cout] or NULL */
  void* wpk;           /* out */
  float* bias_pk;      /* out [CoutP] or NULL */
  int Cout, Cin, KH, KW;
  int KinP;            /* padded reduction channels (multiple of 16) */
  int CoutP;           /* padded rows */
  int dgrad;           /* 0 forward layout, 1 dgrad layout */
  int ps_r;            /* 0/1: none; r>1: NHWC pixel-shuffle permutation on the Cout axis */
  int dtype;
  int rows_layout;     /* 1 (forward, Cin == 64, KH >= 5, Cout <= 4, Cout * KW <= 32, 16-bit): BEHIND the standard layout (KH*KW*KinP*CoutP elements)   */
                       /* wpk also receives KH * 2048 elements in the (kw, co)-rows order of the direct large-kernel forward:           */
                       /* [kh][ci / 16][64 lanes][8]: lane l = MFMA row m = l % 32 = kw * Cout + co (0 beyond KW * Cout), ci = 16 ks + 8 (l / 32) + e */
} srk_pack_args;
int srk_pack_conv_weights(const srk_pack_args* a, srk_stream_t stream);
/* Same, for `n` convolutions in ONE launch: `table` is a DEVICE array of srk_pack_args (a training step re-packs
 * the forward and dgrad layouts of every conv of the model from the updated fp32 parameters).              */
int srk_pack_conv_weights_group(const srk_pack_args* table, int n, srk_stream_t stream);
/* The same launch with blocks that own one 16 x 64-channel tile of one entry each (coalesced reads through LDS).
 * srk_pack_group_tiles (host) fills tile_begin[0 .. n] -- the prefix sums of the entries' tile counts, tile_begin[n] the total --
 * from a HOST copy of the table; the launch takes device copies of both.                                              */
int srk_pack_group_tiles(const srk_pack_args* host_table, int n, int* tile_begin);
int srk_pack_conv_weights_group_tiled(const srk_pack_args* table, const int* tile_begin, int n, int total_tiles, srk_stream_t stream);

/* ---- implicit-GEMM convolution (forward and dgrad) --------------------------------------------
 * Replaces nn.Conv2d(stride 1, padding k//2) + the elementwise ops the reference issues after it:
 * DefaultConv2d (models/common.py:7-30), ReLU (common.py:99-100), `* res_scale` and `res += x`
 * (common.py:106-107, edsr.py:46-47, rcan.py:52-54,72-73,121-122, rdn.py:40,109, wdsr.py:25-26,
 * 49-50,112), nn.PixelShuffle (common.py:133, rdn.py:81,89,92, wdsr.py:88,94), torch.cat slice
 * writes (rdn.py:21,108) and the `add_mean` shift (common.py:58-71).  Epilogue order:
 *     v = acc + bias[co];  if relu: v = max(v,0);  v *= scale;  v += res;
 *     if mask and co >= mask_from: v = (mask > 0) ? v : 0;      (ReLU backward)
 *     v += post_add[c]  (planar mode only);  store.
 * The same kernel computes dgrad when given dgrad-packed weights.                                */
typedef struct {
  const void* x; int x_pitch, x_coff;  /* input NHWC, Cin channels starting at x_coff              */
  int x_ps;                            /* 0/1: plain; r>1: x is stored pixel-shuffled by r, i.e. it is */
                                       /* [N][H*r][W*r][Cin/(r*r)] and channel k = (i*r+j)*C + c     */
  int N, H, W;                         /* conv-space dims ('same' conv: output dims = input dims)    */
  int Cin;                             /* multiple of 16                                              */
  const void* wpk; const float* bias;  /* packed weights [KH*KW][Cin/CH][CoutP][CH]; bias [CoutP]/NULL */
  int CoutP;                           /* multiple of the channel tile chosen by srk_conv_tile()      */
  int Cout;                            /* channels to store (NHWC: multiple of 4, <= CoutP; planar: real) */
  int KH, KW;                          /* 1 or 3 (3x3 with one 64-channel input block in bf16/fp16 runs on   */
                                       /* the weight-stationary persistent kernel, everything else streams)   */
  int relu; float scale;
  const void* res; int res_pitch, res_coff;    /* same addressing mode and dtype as out; NULL = none */
  const void* mask; int mask_pitch, mask_coff; int mask_from;  /* NHWC/NHWC_PS addressing, dtype     */
  void* out; int out_pitch, out_coff; int out_mode; int ps_r;
  const float* post_add;               /* planar: per output channel c, or NULL                      */
  int dtype;
  int cout_real;                       /* the conv's real output channels when wpk carries the rows layout (srk_pack_args.rows_layout), else 0 */
  /* ReLU sign BITS (3x3, 64 -> 64 channels, 16-bit, NHWC out: the weight-stationary kernel; srk_conv_bits_ok): 4 bytes per pixel and
   * 32-channel half, [N*H*W][2] u32; bit i resp. 16 + i of word h <-> channel 32 h + 2 i resp. + 1 > 0 after the ReLU.
   *   relu_bits (out, nullable): written by a conv + ReLU launch (relu = 1, no res / mask / scale) next to its output;
   *   mask_bits (in, nullable, instead of `mask`): the data gradient `v = bit ? v : 0` reads these 8 bytes per pixel instead of the
   *   128-byte activation (ResBlock / RCAB backward, models/common.py:99-100: 75 MB -> 4.7 MB per launch at 256 x 48 x 48).     */
  void* relu_bits; const void* mask_bits;
} srk_conv_args;
/* 1 when srk_conv2d honours relu_bits / mask_bits for these arguments (else they must be NULL) */
int srk_conv_bits_ok(const srk_conv_args* a);
int srk_conv2d(const srk_conv_args* a, srk_stream_t stream);
/* channel tile (32/64/128) the launcher uses for a given number of output channels */
int srk_conv_tile(int Cout);

/* ---- a CHAIN of 3x3 64->64 convolutions in ONE launch, image by image (large batches) -------------------------------
 * Replaces, where the batch fills the chip with whole images (N a multiple of the CU count), the sequence of srk_conv2d launches
 * of a residual trunk -- the 2 x n_resblocks + 1 convolutions of EDSR's body (models/edsr.py:24-31,44-47; ResBlock:
 * models/common.py:74-109) in the forward pass and, given data-gradient packs, their data gradients in the backward pass.
 * A 'same' convolution of an image reads that image only, so the workgroup that owns an image runs the layers on it back
 * to back with no launch boundary and no synchronisation with other workgroups.
 *   layers_host[l] : the arguments srk_conv2d would get for layer l (layer l + 1 normally reads layer l's `out`; `res`,
 *                    `relu_bits`, `mask_bits` may name any buffer written by an EARLIER layer or before the launch);
 *   table_dev      : the same nlayers structs in device memory (srk_upload_small / srk_upload_eager), read by the kernel.
 * Every layer: 16-bit, 3x3, Cin = Cout = CoutP = 64, NHWC output, no pixel shuffle, no `mask` (sign bits only), no
 * post_add; all layers the same N, H, W, dtype and x_pitch.  A layer with KH = KW = 0 is the elementwise `out = x + res` on dense
 * 64-channel tensors (fp32 add, rounded once: the two gradient contributions of a long skip, models/edsr.py:46-47).
 * srk_conv_trunk_ok says whether a table qualifies (0: issue the layers as srk_conv2d launches).  Results are bit-identical to
 * those launches.                                                                                                          */
int srk_conv_trunk_ok(const srk_conv_args* layers_host, int nlayers);
int srk_conv_trunk(const srk_conv_args* layers_host, const void* table_dev, int nlayers, srk_stream_t stream);

/* ---- two chained 3x3 64->64 convolutions in one launch (small batches) ---------------------------
 * Replaces, at the reference's batch of 16 where a layer is one tile per CU and launches dominate, the conv pair of
 * ResBlock (models/common.py:74-109: conv, ReLU, conv, `* res_scale`, `res += x`) and of RCAB (models/rcan.py:33-55),
 * and -- given data-gradient packs -- the backward chain of either:
 *     mid = conv3x3(x, w1) + b1;  if relu_mid: mid = max(mid,0);  mid *= scale_mid;
 *     if mask: mid = (mask > 0) ? mid : 0;            (mid is rounded to the storage dtype, as the two-launch form does)
 *     out = (conv3x3(mid, w2) + b2) * scale_out + res
 * Zero padding of both convs refers to the image, exactly as two srk_conv2d calls.  All tensors NHWC with 64 channels at
 * (pitch, coff); w1 / w2 are srk_pack_conv_weights outputs for Cin = Cout = 64, b1 / b2 the packed (MFMA-row order)
 * biases or NULL.  `mid` (nullable) receives the intermediate (training keeps it for the backward pass).
 * res_from_x = 1 says res IS x (same pointer, pitch, offset): the residual is then taken from the input tile in LDS.
 * Results are bit-identical to the two-launch form.  bf16 / fp16 only.                                              */
typedef struct {
  const void* x; int x_pitch, x_coff;
  int N, H, W;
  const void* w1; const float* b1;
  const void* w2; const float* b2;
  int relu_mid; float scale_mid;
  const void* mask; int mask_pitch, mask_coff;
  void* mid; int mid_pitch, mid_coff;
  float scale_out;
  const void* res; int res_pitch, res_coff; int res_from_x;
  void* out; int out_pitch, out_coff;
  int dtype;
  /* optional channel-attention pooling of the output while it leaves (models/rcan.py:10-29 AdaptiveAvgPool2d numerator and
   * its backward): pool[(n*T + tile)*64 + c] = sum over the tile's pixels of out[.][c] * (pool_aux ? pool_aux[.][c] : 1),
   * T = srk_conv_pair_tiles(1, H, W) partial rows per sample (srk_ca_apply / srk_ca_bwd_apply take them via sums_rows /
   * gsum_rows), summed in a fixed order over the stored (rounded) values                                              */
  float* pool; const void* pool_aux; int pool_aux_pitch, pool_aux_coff;
  /* optional channel-attention step applied to the INPUT while it is loaded (0 = off); x' feeds conv 1 and goes to xo
   * (nullable); a residual must then come from memory (res_from_x = 0).  Same arithmetic and order as the stand-alone launches.
   * ca_mode 1 = srk_ca_bwd_apply: x' = x * s[n][c] + dmean[n][c] (zero outside the image), s / dmean from the MLP backward on
   *   this sample's (ca_gsum [N][ca_gsum_rows][64], ca_sums [N][ca_sums_rows][64], ca_s [N][64], ca_z [N][ca_cr], ca_w1
   *   [ca_cr][64], ca_w2 [64][ca_cr]); ca_slots (nullable): the per-sample parameter-gradient slots [dW1 | db1 | dW2 | db2]
   *   (2*64*ca_cr + ca_cr + 64 floats per sample, written by one workgroup per sample).
   * ca_mode 2 = srk_ca_apply of the PREVIOUS block: x' = x * s[n][c] + ca_x2 with s = sigmoid(W2 relu(W1 mean + b1) + b2), mean
   *   from ca_sums; ca_s_out [N][64] / ca_z_out [N][ca_cr] (nullable) receive s and the hidden activations.            */
  int ca_mode; int ca_cr;
  const float* ca_gsum; int ca_gsum_rows; const float* ca_sums; int ca_sums_rows;
  const float* ca_s; const float* ca_z; const float* ca_w1; const float* ca_w2;
  float* ca_slots;
  void* xo; int xo_pitch, xo_coff;
  const void* ca_x2; int ca_x2_pitch, ca_x2_coff;
  const float* ca_b1; const float* ca_b2; float* ca_s_out; float* ca_z_out;
} srk_conv_pair_args;
int srk_conv_pair(const srk_conv_pair_args* a, srk_stream_t stream);
/* workgroups (14x14 output tiles) such a launch has: the host uses the pair while this is about two per CU or less */
int srk_conv_pair_tiles(int N, int H, int W);

/* ---- two chained pointwise convolutions with the wide intermediate kept on chip -----------------------------------
 * Replaces the opening of WDSR's _Block_B (models/wdsr.py:30-51):
 *     h = relu(conv1x1(x; Cin -> Chid) + b1);   z = conv1x1(h; Chid -> Cmid) + b2
 * (wn(nn.Conv2d(F, 6F, 1)), ReLU, wn(nn.Conv2d(6F, int(.8F), 1))) and its backward
 *     gh = (W2^T gz) * (h > 0);   gx = W1^T gh [+ res]
 * without the Chid-channel tensor ever reaching HBM: the hidden channels are walked in slices of 64 whose activations
 * live in MFMA accumulator registers and become the next GEMM's operand in place.  Pixels are a flat list of P = N*H*W
 * NHWC rows (pitch / channel offset in elements).  Supported shapes: srk_pw_shape_ok(Cin, Chid, CoutP) -- 16-bit storage,
 * (Cin, CoutP) = (128, 128) or (64, 64), Chid a multiple of 64 (WDSR-B at n_feats 128 / 64).
 * srk_pw_pack converts the fp32 matrices of record (w1 [Chid][Cin], w2 [Cmid][Chid], biases) into the two streamed
 * layouts (sizes: srk_pw_pack_bytes(..., bwd = 0 / 1)); h is rounded to the storage dtype exactly like a stored
 * activation would be.  The backward RE-computes the pre-activation with the forward's instruction sequence, so its
 * sign is the forward's ReLU mask bit for bit; with h_out / gh_out (both or neither, [P][Chid] storage dtype) the slices
 * of h and gh are also written for the weight-gradient GEMMs (srk_conv2d_wgrad, KH = KW = 1).                       */
typedef struct {
  const float* w1; const float* b1;     /* [Chid][Cin], [Chid] or NULL */
  const float* w2; const float* b2;     /* [Cmid][Chid], [Cmid] or NULL */
  int Cin, Chid, Cmid, CoutP;           /* CoutP: padded rows of conv 2 (multiple of 64, >= Cmid) */
  void* fwd; void* bwd;                 /* out: srk_pw_pack_bytes(Cin, Chid, CoutP, 0 / 1) bytes each */
  int dtype;
} srk_pw_pack_args;
int srk_pw_shape_ok(int Cin, int Chid, int CoutP);
long long srk_pw_pack_bytes(int Cin, int Chid, int CoutP, int bwd);
int srk_pw_pack(const srk_pw_pack_args* a, srk_stream_t stream);

/* ---- weight normalisation of all weight-normed convs of a model in one launch per direction ----------------------
 * Replaces nn.utils.weight_norm (models/wdsr.py:62, applied to all 51 convs of WDSR): forward w = v * (g / ||v||) per output
 * row (torch._weight_norm, dim 0) and its backward (dv, dg from dw).  `table_dev` is a DEVICE array of jobs (srk_upload_small
 * gets it there); `row0` = number of rows of all earlier jobs, `total_rows` their sum.  forward writes w and inv (1 / ||v||,
 * kept for the backward); backward reads v, g, inv, dw and writes dv, dg.                                            */
typedef struct {
  const float* v; const float* g;   /* [rows][cols], [rows] */
  float* w; float* inv;             /* forward out: [rows][cols], [rows] */
  const float* dw;                  /* backward in */
  float* dv; float* dg;             /* backward out */
  int rows, cols, row0, pad_;
} srk_wn_job;
int srk_weight_norm_group(const srk_wn_job* table_dev, int njobs, int total_rows, int backward, srk_stream_t stream);

/* same as srk_pw_pack for `n` blocks in ONE launch; `table_dev` is a DEVICE array */
int srk_pw_pack_group(const srk_pw_pack_args* table_dev, int n, srk_stream_t stream);

typedef struct {
  const void* x; int x_pitch, x_coff;   /* [P] pixels x Cin channels */
  long long P;
  int Cin, Chid, CoutP;
  int Cout;                             /* channels of z to store (multiple of 8, <= CoutP; channels >= Cmid are zeros) */
  const void* wpk;                      /* srk_pw_pack's `fwd` */
  void* out; int out_pitch, out_coff;
  int dtype;
} srk_pw_args;
int srk_pw_forward(const srk_pw_args* a, srk_stream_t stream);

typedef struct {
  const void* x; int x_pitch, x_coff;   /* the forward's input */
  const void* gz; int gz_pitch, gz_coff; int Cz;   /* gradient of z: Cz stored channels (multiple of 8, <= CoutP) */
  long long P;
  int Cin, Chid, CoutP;
  const void* wpk;                      /* srk_pw_pack's `bwd` */
  const void* res; int res_pitch, res_coff;        /* added to gx (the skip connection's gradient) or NULL */
  void* gx; int gx_pitch, gx_coff;
  void* h_out; void* gh_out;            /* [P][Chid] or NULL (both) */
  int dtype;
} srk_pw_bwd_args;
int srk_pw_backward(const srk_pw_bwd_args* a, srk_stream_t stream);

/* weight gradients of the pointwise pair, again without h / gh in HBM (both are re-computed per 128-pixel tile):
 *     dw1[hid][in] = sum_p gh[p][hid] x[p][in];  db1[hid] = sum_p gh[p][hid];  dw2[z][hid] = sum_p h[p][hid] gz[p][z]
 * and db2[z] = sum_p gz[p][z].  Scratch: nranges = srk_pw_wgrad_ranges(P, Chid) slabs of [Chid][Cin] (dw1p), [Chid][CoutP]
 * (dw2p), [Chid] (db1p) and [CoutP] (db2p) fp32 that the launch fills and then sums in a fixed order.                   */
typedef struct {
  const void* x; int x_pitch, x_coff;
  const void* gz; int gz_pitch, gz_coff; int Cz;
  long long P;
  int Cin, Chid, Cmid, CoutP;
  const void* wpk;                      /* srk_pw_pack's `bwd` */
  float* dw1p; float* dw2p; float* db1p; float* db2p; int nranges;   /* db2p / db2: both or neither */
  float* dw1; float* db1; float* dw2; float* db2;   /* out: [Chid][Cin], [Chid] (nullable), [Cmid][Chid], [Cmid] (nullable) */
  int dtype;
} srk_pw_wgrad_args;
int srk_pw_wgrad_ranges(long long P, int Chid);
int srk_pw_wgrad(const srk_pw_wgrad_args* a, srk_stream_t stream);

/* ---- weight / bias gradient -------------------------------------------------------------------
 * Replaces autograd's conv weight-gradient for the convs above:
 *     dwp[slab][tap][ci][co] = sum over the slab's pixels of x[n][y+kh-ph][x+kw-pw][ci] * dy[n][y][x][co]
 *     dbp[slab][co]          = sum over the slab's pixels of dy
 * dwp/dbp are fp32 scratch that needs no zeroing: every workgroup STORES its partial sum to its own slab, and
 * srk_wgrad_finalize sums the slabs in a fixed order and converts to OIHW (bitwise reproducible, every dtype). */
typedef struct {
  const void* x; int x_pitch, x_coff; int x_ps;
  const void* dy; int dy_pitch, dy_coff; int dy_ps;
  int N, H, W;
  int Cin, Cout;            /* both multiples of 16 (padded storage channels)                     */
  int KH, KW;
  float* dwp;               /* fp32 scratch: nslabs x [KH*KW][Cin][Cout]                          */
  float* dbp;               /* fp32 scratch: nslabs x [Cout], or NULL                             */
  int nslabs;               /* value returned by srk_wgrad_slabs() for these arguments (> 0):     */
                            /* every workgroup stores its partial sum to its own slab (no         */
                            /* atomics, no zeroing, bitwise reproducible), fp32 included          */
  int dtype;
  int cout_real;            /* the conv's real output channels (<= Cout), or 0 = unknown: large kernels   */
                            /* with few of them (cout_real * KW <= 32) put (kw, co) pairs on the MFMA columns */
} srk_wgrad_args;
int srk_conv2d_wgrad(const srk_wgrad_args* a, srk_stream_t stream);
/* number of slabs srk_conv2d_wgrad will write for these arguments (> 0 for every shape it takes; the generic kernel of fp32 and of
 * refused 16-bit shapes writes at most 256 / (channel-block pairs): <= 9.4 MB of scratch per fp32 3x3 launch whatever Cin and Cout) */
int srk_wgrad_slabs(const srk_wgrad_args* a);
/* channels per (tap, ci) row of a slab (and of a dbp row): Cout, or 4 for the compact slabs of large kernels with few real output
 * channels (cout_real <= 4); the caller sizes dwp / dbp and sets srk_wgrad_finalize's CoutP with it */
int srk_wgrad_slab_cout(const srk_wgrad_args* a);

typedef struct {
  const float* dwp; const float* dbp;   /* from srk_conv2d_wgrad                                 */
  int nslabs;                           /* slabs to sum (0 or 1: a single slab)                  */
  float* dw; float* db;                 /* OIHW fp32 [Cout][Cin][KH][KW], [Cout]; db may be NULL */
  int Cout, Cin, KH, KW;                /* real sizes                                            */
  int CinP, CoutP;                      /* padded sizes used by dwp                              */
  int ps_r;                             /* channel permutation of SRK_OUT_NHWC_PS on Cout        */
  float scale;                          /* multiplies the result (res_scale, loss un-scaling)    */
  int accumulate;                       /* 0: dw = v, 1: dw += v                                 */
} srk_wgrad_fin_args;
int srk_wgrad_finalize(const srk_wgrad_fin_args* a, srk_stream_t stream);

/* ---- grouped weight gradient: every 3x3 weight gradient of a training step in ONE dispatch ------------------------
 * The weight gradients of a step are independent of each other; per layer they are 37 (EDSR-baseline) to 411 (RCAN)
 * launches of only 144 tiles at the reference's batch of 16 (configs/train_default_sr.yml:3).  The host side defers
 * them to the end of backward (torch.autograd's final callback) and issues two launches: this kernel, which walks a
 * device table of jobs with equal tile counts per workgroup whatever the layer, and srk_wgrad_finalize_group.
 *   srk_wgrad_group_ok   : 1 when `a` can be a job (16-bit, 3x3, a shape the DMA slab kernel "wgrad_ws" takes).
 *   srk_wgrad_group_plan : in : jobs[i] with dbp != NULL where a bias gradient is wanted; `scratch` NULL = sizing pass.
 *                          out: jobs[i].nslabs, *nblocks, *scratch_floats; with `scratch` (device, fp32, that many floats)
 *                               also jobs[i].dwp / dbp (slab regions inside it) and, when given, the HOST images of the
 *                               device tables: table_host [n * srk_wgrad_group_job_bytes()], block_job_host [nblocks].
 *   srk_conv2d_wgrad_group: the launch; both tables in DEVICE memory (srk_upload_small gets them there).           */
int srk_wgrad_group_ok(const srk_wgrad_args* a);
int srk_wgrad_group_job_bytes(void);
int srk_wgrad_group_plan(srk_wgrad_args* jobs, int n, float* scratch, void* table_host, int* block_job_host,
                         int* nblocks, long long* scratch_floats);
int srk_conv2d_wgrad_group(const void* table_dev, const int* block_job_dev, int nblocks, int dtype, srk_stream_t stream);
/* `n` finalizations of 3x3 gradients (KH = KW = 3) in one launch: `table_dev` is a DEVICE array of srk_wgrad_fin_args,
 * `blocks_per_job` workgroups each; slabs are summed in slab order (bitwise reproducible) */
int srk_wgrad_finalize_group(const srk_wgrad_fin_args* table_dev, int n, int blocks_per_job, srk_stream_t stream);
/* Copies a small HOST table (<= 4 MiB) to 16-byte-aligned DEVICE memory through kernel arguments: capturable into a
 * hipGraph (a replay rewrites the same bytes), no pinned staging buffer.                                          */
int srk_upload_small(void* dst_dev, const void* src_host, long long nbytes, srk_stream_t stream);
/* The same upload for a table that a hipGraph UNDER CAPTURE will own and whose memory the capture site keeps alive as long as the graph
 * (ops.static_tables): the bytes are written once, now, on a stream of the library's own (no graph nodes); srk_upload_fence() -- after the
 * capture has ended, before the first replay -- waits for them.  srk_upload_prepare() creates that stream and must run outside any capture.
 * The stream belongs to the CURRENT device of the calling thread (one per device, created once under a mutex): all three calls of one table
 * must be made with the table's device current.                                                                                          */
int srk_upload_prepare(void);
int srk_upload_eager(void* dst_dev, const void* src_host, long long nbytes);
int srk_upload_fence(void);

/* ---- input unfold (model boundary) -----------------------------------------------------------------
 * Head convs 3->F (edsr.py:21-22, rcan.py:92-93, rdn.py:57-58, wdsr.py:69-71) and WDSR's 5x5 skip conv
 * (wdsr.py:90-94) have Cin <= 4: too thin for a 16-channel MFMA K-chunk.  The boundary kernel fuses the
 * input mean shift (common.py:58-71 sign=-1, wdsr.py:103-105), the NCHW fp32 -> NHWC conversion and an
 * im2col of the K x K window:
 *     dst[n][y][x][ci*KH*KW + kh*KW + kw] = x[n][ci][y+kh-ph][x+kw-pw] - sub[ci]      (0 outside the image)
 * so the conv becomes a 1x1 conv over Cin*KH*KW (padded to 16) channels whose weight matrix is
 * w.reshape(Cout, Cin*KH*KW) -- the OIHW parameter itself -- and runs through srk_conv2d /
 * srk_conv2d_wgrad like every other layer.                                                          */
typedef struct {
  const float* x;           /* NCHW fp32 [N][Cin][H][W]                                            */
  const float* sub;         /* per-input-channel value subtracted before the conv, or NULL         */
  void* dst; int dst_pitch, dst_coff;
  int N, Cin, H, W, KH, KW;
  int Kstore;               /* channels written: >= Cin*KH*KW, multiple of 16, extra are zero      */
  int dtype;
} srk_unfold_args;
int srk_unfold_nchw(const srk_unfold_args* a, srk_stream_t stream);

/* ---- layout conversion at the model boundary ------------------------------------------------------
 * NCHW fp32 <-> NHWC dtype.  `ps_r` > 1 on to_nhwc un-shuffles: dst[n][y][x][c*r*r+i*r+j] =
 * src[n][c][y*r+i][x*r+j] (the adjoint of the fused PixelShuffle store in planar mode).        */
typedef struct {
  const float* src; void* dst; int dst_pitch, dst_coff;
  int N, C, H, W;           /* dst dims: C channels (padded with zeros up to Cstore), H x W      */
  int Cstore; int ps_r; float scale; int dtype;
} srk_to_nhwc_args;
int srk_nchw_to_nhwc(const srk_to_nhwc_args* a, srk_stream_t stream);

typedef struct {
  const void* src; int src_pitch, src_coff; float* dst;
  int N, C, H, W; int dtype;
} srk_to_nchw_args;
int srk_nhwc_to_nchw(const srk_to_nchw_args* a, srk_stream_t stream);

/* ---- RCAN channel attention -----------------------------------------------------------------------
 * CALayer.forward (models/rcan.py:10-29) fused with RCAB's `res += x` (rcan.py:52-54):
 *   sums[n][s][c] = sum over the pixels of block s of t (or t*u)   (srk_ca_pool: wave/LDS reductions, ONE plain store
 *                   per block and channel -- S = srk_ca_splits(N, HW) blocks per sample, no atomics, nothing to zero,
 *                   bitwise reproducible; the consumers add the S partials in block order)
 *   z = relu(W1 mean + b1); s = sigmoid(W2 z + b2); out = t * s + res    (srk_ca_apply)
 * and its backward (srk_ca_pool with u = g, srk_ca_bwd_apply).  W1:[Cr][C], W2:[C][Cr] are the raw
 * fp32 parameters conv_du.0.weight / conv_du.2.weight.                                         */
int srk_ca_splits(int N, int HW);
typedef struct {
  const void* t; int t_pitch, t_coff;
  const void* u; int u_pitch, u_coff;   /* NULL: plain sum of t; else sum of t*u (backward)      */
  float* sums;                          /* [N][S][C] fp32 partial sums, S = srk_ca_splits(N, HW) */
  int N, HW, C; int dtype;
} srk_ca_pool_args;
int srk_ca_pool(const srk_ca_pool_args* a, srk_stream_t stream);

typedef struct {
  const void* t; int t_pitch, t_coff;
  const void* res; int res_pitch, res_coff;     /* nullable */
  const float* sums;                    /* [N][S][C] from srk_ca_pool                            */
  const float* w1; const float* b1; const float* w2; const float* b2;
  float* s_out; float* z_out;           /* [N][C], [N][Cr] saved for backward (nullable)         */
  void* out; int out_pitch, out_coff;
  int N, HW, C, Cr; int dtype;
  int sums_rows;                        /* partial rows per sample in `sums`; 0 = srk_ca_splits(N, HW) (srk_ca_pool's)   */
} srk_ca_apply_args;
int srk_ca_apply(const srk_ca_apply_args* a, srk_stream_t stream);

typedef struct {
  const void* g; int g_pitch, g_coff;   /* gradient w.r.t. the CA output (t*s)                   */
  const float* gsum;                    /* [N][S][C] = partial sums of g*t from srk_ca_pool(t,u=g) */
  const float* sums; const float* s; const float* z;   /* saved by forward                      */
  const float* w1; const float* w2;
  float* dw1; float* db1; float* dw2; float* db2;      /* out: PER-SAMPLE contributions; each pointer is the   */
                                        /* sample-0 slot, sample n is 2*C*Cr + Cr + C floats further; the  */
                                        /* caller sums over n (fixed order: reproducible)                  */
  void* gt; int gt_pitch, gt_coff;      /* out: gradient w.r.t. t = g*s + dmean/HW               */
  int N, HW, C, Cr; int dtype;
  int sums_rows, gsum_rows;             /* partial rows per sample in `sums` / `gsum`; 0 = srk_ca_splits(N, HW)          */
} srk_ca_bwd_args;
int srk_ca_bwd_apply(const srk_ca_bwd_args* a, srk_stream_t stream);
/* dst[i] = sum over r < n of src[r*k + i] (row order: reproducible) for `njobs` entries of a DEVICE table in one launch: the
 * sums over the batch of the per-sample slots srk_ca_bwd_apply writes, for every CALayer of a backward pass at once
 * (replaces the conv_du weight / bias gradient reductions autograd performs per layer, models/rcan.py:10-29).        */
typedef struct { const float* src; float* dst; int n; int k; } srk_rowsum_job;
int srk_rowsum_group(const srk_rowsum_job* table_dev, int njobs, int max_k, srk_stream_t stream);

/* ---- data step feeding the path ------------------------------------------------
 * _SRDataset._get_item / _get_patch in 'train' mode (srdata.py:64-91,137-169): crop an LR patch and the matching
 * HR patch, rotate both counter-clockwise by rot*90 degrees, horizontal flip, vertical flip, uint8 -> float / 255,
 * HWC -> CHW.  One launch for a whole batch: `table` is a DEVICE array of per-sample descriptors (images stay on
 * the GPU as uint8 HWC), outputs are the NCHW fp32 batch tensors that SRModel.training_step consumes.        */
typedef struct {
  const uint8_t* lr; const uint8_t* hr;   /* uint8 [H][W][C] images of this sample (device)               */
  int lr_h, lr_w, hr_h, hr_w;
  int top, left;                          /* LR patch origin (row, column); the HR origin is scale * that  */
  int rot;                                /* 0..3 quarter turns counter-clockwise                          */
  int hflip, vflip;
} srk_patch_desc;
typedef struct {
  const srk_patch_desc* table; int N; int C; int patch_lr; int scale;
  float* lr_out;                          /* [N][C][patch_lr][patch_lr]                                    */
  float* hr_out;                          /* [N][C][patch_lr*scale][patch_lr*scale]                        */
} srk_patch_args;
int srk_sample_patches(const srk_patch_args* a, srk_stream_t stream);

/* ---- metric core on the device ---------------------------------------------------
 * validation_step clamps both images to [0,1] and calls piq.psnr (srmodel.py:224-232,582).  This reduction
 * returns per image the sum of squared differences of the clamped images and the element count, either over all
 * channels (RGB PSNR, the reference's definition) or over the BT.601 luma with a `shave`-pixel border removed
 * (PSNR-Y, the convention BASELINE.json names).  PSNR = 10 log10(count / sse) is left to the caller.        */
typedef struct {
  const float* sr; const float* hr;       /* NCHW fp32                                                     */
  int N, C, H, W;
  int luma;                               /* 0: all channels; 1: BT.601 Y of the 3 channels                */
  int shave;                              /* border removed on every side (luma or not)                    */
  double* sse;                            /* [N] sums, caller-zeroed                                       */
} srk_sse_args;
int srk_image_sse(const srk_sse_args* a, srk_stream_t stream);

/* ---- L1 loss of the training step (reference srmodel.py:160-171 -> F.l1_loss, 'mean' reduction), fused:
 * forward reads sr and hr once, writes per-block partial sums of |sr - hr| (summed in a fixed order by the caller:
 * reproducible) and the sign of (sr - hr) as int8; backward turns the sign map into the gradient
 * sign * (*gout) * scale without touching sr / hr again.  gout is a DEVICE scalar (no host sync, graph-capturable). */
typedef struct srk_l1_args {
  const float* sr;                        /* forward: [n] ; backward: unused                                */
  const float* hr;
  long long n;
  signed char* sign;                      /* [n] sign(sr - hr) in {-1, 0, 1}: written by forward, read by backward */
  double* partial;                        /* forward: [srk_l1_blocks(n)] partial sums                       */
  const float* gout;                      /* backward: device scalar                                        */
  float scale;                            /* backward: weight / n                                           */
  float* grad;                            /* backward: [n]                                                  */
} srk_l1_args;
int srk_l1_blocks(long long n);
int srk_l1_loss_fwd(const srk_l1_args* a, srk_stream_t stream);
int srk_l1_loss_bwd(const srk_l1_args* a, srk_stream_t stream);
/* *out = (partial[0] + ... + partial[nb-1]) / n: the forward's partial sums -> the loss value, one launch */
int srk_l1_loss_mean(const double* partial, int nb, long long n, float* out, srk_stream_t stream);

/* ---- FLIP loss / metric (reference losses/flip.py, srmodel.py:35,49; Andersson et al., HPG 2020), csrc/flip.hip ------------------
 * Forward: one workgroup per (image, 32x32 tile) with a 10-pixel halo (replicate-clamped loads): sRGB -> linear -> XYZ -> YCxCz of
 * both images, the separable CSF filters (radius 10) of the three opponent channels and the edge / point detectors (radius 9) on
 * the unfiltered luminance, then the per-pixel colour and feature errors and err = C ** (1 - F).  Writes one double partial sum
 * per workgroup (summed in a fixed order: reproducible), optionally the error map and, for a gradient, the 7 per-pixel adjoints of
 * err for a unit upstream gradient: d err / d(filtered test Y, Cx, Cz) and d err / d(test edge x, edge y, point x, point y).
 * Pixels whose colour error is 0 get zero adjoints, and a zero feature difference a zero feature adjoint (the reference's
 * autograd gives NaN there; sr_amd/flip.py states the convention).
 * Backward: the transposed separable filters (the adjoint of `replicate` folds the outside taps onto the edge pixel), the
 * feature path into Y, the YCxCz <- XYZ <- linear <- sRGB Jacobian with the input clamp's mask, times (*gout) * scale.
 * The constant table (SRK_FLIP_TABLE_FLOATS fp32, layout in sr_amd/flip.py) is built on the host and lives on the device.
 * NCHW fp32, C = 3, N <= 65535, any H, W >= 1. ---------------------------------------------------------------------------- */
#define SRK_FLIP_TABLE_FLOATS 176
#define SRK_FLIP_ADJ_CHANNELS 7
typedef struct srk_flip_args {
  const float* sr;                        /* test image [N][3][H][W] (forward and backward)                                  */
  const float* hr;                        /* reference image [N][3][H][W] (forward)                                          */
  int N, H, W;
  const float* table;                     /* [SRK_FLIP_TABLE_FLOATS] device constants                                        */
  double* partial;                        /* forward: [srk_flip_blocks(N, H, W)] partial sums of err                         */
  float* err;                             /* forward, optional: [N][H][W] error map                                          */
  float* adj;                             /* forward writes (optional), backward reads: [N][7][H][W]                        */
  const float* gout;                      /* backward: device scalar                                                         */
  float scale;                            /* backward: 1 / (N H W)                                                           */
  float* grad;                            /* backward: [N][3][H][W] d loss / d sr                                            */
} srk_flip_args;
int srk_flip_blocks(int N, int H, int W);
int srk_flip_fwd(const srk_flip_args* a, srk_stream_t stream);
int srk_flip_bwd(const srk_flip_args* a, srk_stream_t stream);
/* *out = (partial[0] + ... + partial[nb-1]) / n (the forward's partial sums -> the mean error), one launch */
int srk_flip_mean(const double* partial, int nb, long long n, float* out, srk_stream_t stream);

/* ---- HaarPSI loss (piq 0.7.0 HaarPSILoss with its defaults; reference srmodel.py:36), csrc/haarpsi.hip ------------------------
 * x = clamp(sr, 0, 1) (test), y = hr (reference), both x255; C == 3: YIQ per pixel, C == 1: the channel is Y.  Subsampled by a
 * bottom / right zero pad of p = max(H % 2, W % 2) and a 2x2 / stride-2 mean (H' = (H + p) / 2, W' = (W + p) / 2).  Haar
 * coefficients of Y' at k = 2, 4, 8 (zero pad k/2 - 1 top / left, k/2 bottom / right), weights w_o = max(|h_8^o x|, |h_8^o y|),
 * similarities sim_o = (S(h_2^o) + S(h_4^o)) / 2, S(u, v) = (2uv + 30) / (u^2 + v^2 + 30 + 2^-23) on magnitudes; for C == 3 also
 * the I / Q term on a bottom / right padded 2x2 / stride-1 mean, with w_2 = (w_0 + w_1) / 2.  Per image
 * r_n = (sum sigma(4.2 sim) w + eps) / (sum w + eps), eps = 2^-23; h_n = (logit(r_n) / 4.2)^2; loss = 1 - mean h_n.
 * Forward: one workgroup per (image, 16x16 half-res tile) -> two doubles per tile (fixed slots, no atomics).  Finalize: one
 * workgroup, fixed-order fp64 sums -> loss, index and per-image factors.  Backward: recomputes the tile on a 7-pixel halo from
 * the subsampled planes the forward kept; d loss / d sr times *gout (device scalar: no host sync), zero where sr lies outside
 * [0, 1].  hr gets no gradient and is not range-checked.  NCHW fp32, C in {1, 3}, H, W >= 16, N <= 65535. ---------------------------------------------------------- */
typedef struct srk_haarpsi_args {
  const float* sr;                        /* test image [N][C][H][W] (forward, backward; clamped on load)                    */
  const float* hr;                        /* reference image [N][C][H][W] (forward)                                          */
  int N, C, H, W;
  double* partial;                        /* [srk_haarpsi_tiles(N, H, W)][2]: per tile sum sigma(alpha sim) w, sum w        */
  float* planes;                          /* forward writes (optional), backward reads: [N][C == 3 ? 6 : 2][H'][W'] Y'x, Y'y  */
                                          /* (and I'x, Q'x, I'y, Q'y): the subsampled x255 planes of both images            */
  float* stats;                           /* [N][4]: r_n, 1 / (W_n + eps), d loss / d r_n for a unit upstream gradient, h_n  */
  float* loss;                            /* finalize: device scalar 1 - index                                               */
  float* index;                           /* finalize, optional: device scalar mean h_n                                      */
  const float* gout;                      /* backward: device scalar                                                         */
  float* grad;                            /* backward: [N][C][H][W] d loss / d sr                                            */
} srk_haarpsi_args;
/* forward tiles over the whole batch (N x per-image tiles), or -1 when the sizes are refused (H or W < 16) */
int srk_haarpsi_tiles(int N, int H, int W);
int srk_haarpsi_fwd(const srk_haarpsi_args* a, srk_stream_t stream);
int srk_haarpsi_finalize(const srk_haarpsi_args* a, srk_stream_t stream);
int srk_haarpsi_bwd(const srk_haarpsi_args* a, srk_stream_t stream);

/* ---- SSIM loss (piq.SSIMLoss with piq.ssim's defaults; "0.16*l1+0.84*ssim" of Zhao et al. 2017), csrc/ssim_loss.hip --------------
 * x = clamp(sr, 0, 1) (test), y = hr (reference).  Both are average-pooled by f = max(1, round(min(H, W) / 256)) (Python's round;
 * Hp = H / f, Wp = W / f, remainder rows / columns dropped), filtered with the separable 11-tap Gaussian (sigma 1.5) over the
 * valid (Hp-10) x (Wp-10) map: S = (2 mu_x mu_y + c1)(2 s_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(s_xx + s_yy + c2)), c1 = 1e-4,
 * c2 = 9e-4; loss = 1 - mean of S over the map, the channels and the images (srk_image_ssim's value on in-range input).
 * Forward: one workgroup per (plane, 16x16 map tile) -> one double per tile in its own slot (no atomics).  Finalize: one workgroup,
 * the fixed-order fp64 sum -> loss.  Backward: one workgroup per (plane, 16x32 pooled-pixel tile) recomputes the moments on a
 * 10-pixel halo from sr and hr, d loss / d sr times *gout (device scalar: no host sync), each pixel of an f x f block taking
 * 1 / f^2 of its pooled pixel's gradient, zero where sr lies outside [0, 1].  The dropped remainder rows / columns of grad are
 * NOT written: the caller zeroes them.  hr gets no gradient and is not range-checked.  NCHW fp32, any C >= 1, Hp, Wp >= 11,
 * N * C * (tiles per plane) < 2^31. ------------------------------------------------------------------------------------------- */
typedef struct srk_ssim_loss_args {
  const float* sr;                        /* test image [N][C][H][W] (forward, backward; clamped on load)                    */
  const float* hr;                        /* reference image [N][C][H][W] (forward, backward)                                */
  int N, C, H, W;
  double* partial;                        /* [srk_ssim_loss_tiles(N, C, H, W)]: per forward tile, the sum of S               */
  float* loss;                            /* finalize: device scalar 1 - SSIM                                                */
  const float* gout;                      /* backward: device scalar                                                         */
  float* grad;                            /* backward: [N][C][H][W] d loss / d sr                                            */
} srk_ssim_loss_args;
/* forward tiles over the whole batch (N * C planes x tiles per plane), or -1 when the sizes are refused */
int srk_ssim_loss_tiles(int N, int C, int H, int W);
int srk_ssim_loss_fwd(const srk_ssim_loss_args* a, srk_stream_t stream);
int srk_ssim_loss_finalize(const srk_ssim_loss_args* a, srk_stream_t stream);
int srk_ssim_loss_bwd(const srk_ssim_loss_args* a, srk_stream_t stream);

/* ---- MS-SSIM loss (piq.MultiScaleSSIMLoss with piq.multi_scale_ssim's defaults; "0.16*l1+0.84*ms_ssim" of Zhao et al. 2017),
 * csrc/ms_ssim_loss.hip.  x = clamp(sr, 0, 1) (test), y = hr (reference); the pyramid, the maps and the per-level means cs_k, ss_k
 * are srk_ms_ssim's (below).  m_k = cs_k (k < 4), m_4 = ss_4; per (image, channel) plane v = prod_k max(m_k, 0)^w_k with the weights
 * 0.0448, 0.2856, 0.3001, 0.2363, 0.1333; loss = 1 - mean of v over channels and images.  H, W >= 161, H * W <= 2^24, any C >= 1,
 * N * C * (blocks per plane of any launch) < 2^31: anything else is refused with -1.
 * Forward: four pooling launches (the clamp of sr folded into the reads of level 0) fill `workspace` with levels 1-4 of both images,
 * then one launch over the 16x16 map tiles of all five levels writes (sum ss, sum cs) per tile to a fixed slot of `partials`.
 * Finalize: one workgroup, fixed-order fp64 sums -> `loss`, and table[plane][k] = w_k v / (m_k count_k N C), the factor the backward
 * scales level k's adjoint by; all five are 0 for a plane with any m_k <= 0 (v = 0 there; piq's relu(m)^w has an infinite slope at 0
 * and its autograd returns NaN: here such a plane gets a zero gradient).
 * Backward: one launch per level, level 4 first.  One workgroup per (plane, 16x32 pixel tile of level k) recomputes the moments on a
 * 10-pixel halo from the pyramid, applies the transposed filter to the adjoint of cs (ss at level 4) times -table[plane][k],
 * adds 1/4 of the gradient of its parent pixel ((i + p) / 2, (j + p) / 2) of level k+1 (nothing when
 * that lies outside level k+1: the row / column the pooling's floor drops; twice that share on row / column 0 when p = 1: the
 * replicated pad) and writes level k's gradient once, levels 1-4 (per unit of the upstream gradient) into `gwork`, level 0 times
 * *gout (device scalar: no host sync; applied once, so grad is linear in it to the last bit) under the clamp's mask (zero where sr
 * lies outside [0, 1]) into `grad`.  Gather form: no atomics; bit-reproducible.  hr gets no gradient and is not range-checked.
 * NCHW fp32.  `workspace`, `table` and sr / hr must be the forward's when the backward runs. ----------------------------------- */
typedef struct srk_ms_ssim_loss_args {
  const float* sr;                        /* test image [N][C][H][W] (forward, backward; clamped on load)                    */
  const float* hr;                        /* reference image [N][C][H][W] (forward, backward)                                */
  int N, C, H, W;
  float* workspace;                       /* srk_ms_ssim_loss_workspace_bytes(N, C, H, W) bytes: levels 1-4 of both images   */
  double* partials;                       /* [N*C][srk_ms_ssim_loss_tiles(...)][2], 16-byte aligned: (sum ss, sum cs)        */
  float* table;                           /* [N*C][5]: finalize writes, backward reads                                       */
  float* loss;                            /* finalize: device scalar 1 - MS-SSIM                                             */
  const float* gout;                      /* backward: device scalar                                                         */
  float* gwork;                           /* backward: half the workspace's bytes, the gradients of levels 1-4 of x          */
  float* grad;                            /* backward: [N][C][H][W] d loss / d sr                                            */
} srk_ms_ssim_loss_args;
/* bytes of the pyramid workspace (a multiple of 256; srk_ms_ssim_workspace_bytes' value), or -1 when the sizes are refused */
long long srk_ms_ssim_loss_workspace_bytes(int N, int C, int H, int W);
/* map tiles per plane over all five levels (srk_ms_ssim_tiles' value), or -1 when the sizes are refused; first (nullable)
 * receives the 6 level boundaries */
int srk_ms_ssim_loss_tiles(int N, int C, int H, int W, int* first);
int srk_ms_ssim_loss_fwd(const srk_ms_ssim_loss_args* a, srk_stream_t stream);
int srk_ms_ssim_loss_finalize(const srk_ms_ssim_loss_args* a, srk_stream_t stream);
int srk_ms_ssim_loss_bwd(const srk_ms_ssim_loss_args* a, srk_stream_t stream);

/* ---- GMSD loss and metric (gradient magnitude similarity deviation, Xue, Zhang, Mou, Bovik 2014; piq.GMSDLoss), csrc/gmsd.hip -----
 * x = clamp(sr, 0, 1) (test), y = hr (reference), C = 1 or 3.  Luma Y = 0.299 R + 0.587 G + 0.114 B (C = 3) or the plane (C = 1);
 * p = max(H % 2, W % 2) rows / columns of zeros at the bottom / right, then the 2x2 stride-2 average (floor): Hd = (H + p) / 2,
 * Wd = (W + p) / 2; Prewitt taps [[-1, 0, 1]] x 3 / 3 and their transpose as a cross-correlation with zero padding 1;
 * a = |grad x|, b = |grad y|, GMS = (2ab + c) / (a^2 + b^2 + c), c = 170 / 255^2; GMSD_n = the population standard deviation of GMS
 * over the Hd x Wd positions of image n; loss = mean over n of GMSD_n (0 is a perfect match).
 * Forward: one workgroup per (image, 16x32 tile of the pooled map) stages the pooled luma of both images with a 1-position halo in
 * LDS and writes (sum d, sum d^2) of d = GMS - 1 = -(a - b)^2 / (a^2 + b^2 + c) as two doubles into its own slot (no atomics).
 * Finalize: per image the fixed-order fp64 sums -> stats[n] = (mean of d, GMSD_n), then the fixed-order mean over n -> loss.
 * Backward: one workgroup per (image, 16x32 tile of pooled pixels = 32x64 pixels of sr) recomputes the pooled luma on a 2-position
 * halo and a, b, GMS on a 1-position halo, d loss / d GMS = (d - mean_n) / (Hd Wd GMSD_n N) from `stats`, through d GMS / d a, the
 * transposed taps, the 1/4 of the pool, the luma coefficient and the clamp's mask (zero where sr lies outside [0, 1]), times *gout
 * (device scalar: no host sync; applied once, last, so grad is linear in it to the last bit).  Every element of grad is written.  Where grad x = 0 the square root's derivative is taken as 0,
 * and an image with GMSD_n = 0 gets a zero gradient.  hr gets no gradient and is not range-checked.  NCHW fp32,
 * N * (tiles per image) < 2^31. ------------------------------------------------------------------------------------------------ */
typedef struct srk_gmsd_args {
  const float* sr;                        /* test image [N][C][H][W] (forward, backward; clamped on load)                    */
  const float* hr;                        /* reference image [N][C][H][W] (forward, backward)                                */
  int N, C, H, W;
  double* partial;                        /* [srk_gmsd_tiles(N, C, H, W)][2]: per forward tile (sum d, sum d^2), d = GMS - 1 */
  float* stats;                           /* [N][2]: finalize writes (mean of d, GMSD_n), backward reads                     */
  float* loss;                            /* finalize: device scalar, the mean of GMSD_n                                     */
  const float* gout;                      /* backward: device scalar                                                         */
  float* grad;                            /* backward: [N][C][H][W] d loss / d sr                                            */
} srk_gmsd_args;
/* forward tiles over the whole batch (N images x tiles per image), or -1 when the sizes are refused */
int srk_gmsd_tiles(int N, int C, int H, int W);
int srk_gmsd_fwd(const srk_gmsd_args* a, srk_stream_t stream);
int srk_gmsd_finalize(const srk_gmsd_args* a, srk_stream_t stream);
int srk_gmsd_bwd(const srk_gmsd_args* a, srk_stream_t stream);

/* ---- pixel losses: Charbonnier, Huber, smooth-L1, Barron's general robust loss with fixed alpha and c, and the PSNR loss,
 * csrc/pixel_loss.hip.  d = sr - hr, nothing is clamped, mean reduction; hr gets no gradient.
 * Elementwise family, `kind` (uniform per launch: the kernels are instantiated per kind, no per-element branch on it), parameters p0, p1:
 *   CHARBONNIER   sqrt(d^2 + p0^2)                                         psi = d / sqrt(d^2 + p0^2)            p0 = eps
 *   HUBER         |d| <= p0 ? d^2 / 2 : p0 (|d| - p0 / 2)                  psi = |d| <= p0 ? d : p0 sign(d)      p0 = delta
 *   SMOOTH_L1     |d| <  p0 ? d^2 / (2 p0) : |d| - p0 / 2                  psi = |d| <  p0 ? d / p0 : sign(d)    p0 = beta (0: L1)
 *   ROBUST_*      rho(d; alpha, c) of Barron (CVPR 2019, eq. 13), z = (d / c)^2, b = |alpha - 2|, p0 = alpha, p1 = c; the host picks
 *                 the exact case:  _A2 (alpha = 2): z / 2;  _A0 (alpha = 0): log1p(z / 2);  _NEG_INF: -expm1(-z / 2);
 *                 _GENERAL (any other alpha): (b / alpha) expm1((alpha / 2) log1p(z / b)), the form that does not cancel in
 *                 fp32 for small |d|;  psi = (d / c^2) (z / b + 1)^(alpha / 2 - 1) and its limits d / c^2, (d / c^2) / (z / 2 + 1),
 *                 (d / c^2) exp(-z / 2).  The kinds are told apart on the fp32 alpha this struct carries; _GENERAL needs alpha, b,
 *                 1 / b and b / alpha, and every robust kind c^2 and 1 / c^2, to be finite normal fp32 numbers (the caller's check).
 * Forward: float4 grid-stride loads of both images, per thread an fp32 sum of at most four values, then double; wave shuffle + LDS;
 * one double per block in its own slot (no atomics), a scalar tail for n % 4; srk_l1_loss_mean over the srk_pixel_loss_blocks(n)
 * partials gives the loss.  Backward: grad = (*gout) * scale * psi(d), gout a DEVICE scalar (no host sync, capturable), psi
 * RECOMPUTED from the two saved images: forward moves 8 B per element, backward 12 B, and nothing HR-sized is allocated besides
 * grad (storing psi in the forward would move 12 B and 8 B, the same 20 B, and hold one more HR-sized buffer from forward to
 * backward).  sr, hr and grad 16-byte aligned. */
enum { SRK_PIXEL_CHARBONNIER = 0, SRK_PIXEL_HUBER = 1, SRK_PIXEL_SMOOTH_L1 = 2, SRK_PIXEL_ROBUST_A2 = 3, SRK_PIXEL_ROBUST_A0 = 4,
       SRK_PIXEL_ROBUST_NEG_INF = 5, SRK_PIXEL_ROBUST_GENERAL = 6 };
#define SRK_PIXEL_LOSS_BLOCK_ELEMS 1024
#define SRK_PIXEL_LOSS_BLOCKS_MAX 2048
typedef struct srk_pixel_loss_args {
  const float* sr;                        /* [n] (forward, backward)                                                          */
  const float* hr;                        /* [n] (forward, backward)                                                          */
  long long n;
  int kind;                               /* SRK_PIXEL_*                                                                      */
  float p0, p1;                           /* the kind's parameters (above); an unused one is ignored                          */
  double* partial;                        /* forward: [srk_pixel_loss_blocks(n)] partial sums                                 */
  const float* gout;                      /* backward: device scalar                                                          */
  float scale;                            /* backward: 1 / n                                                                  */
  float* grad;                            /* backward: [n] d loss / d sr                                                      */
} srk_pixel_loss_args;
/* blocks of either launch, the length of `partial`: ceil(floor(n / 4) / 256), the float4s over the 256 threads of a block, kept in
 * [1, SRK_PIXEL_LOSS_BLOCKS_MAX] (n = 1025 is one block: the grid-stride loop and block 0's tail cover every element) */
int srk_pixel_loss_blocks(long long n);
int srk_pixel_loss_fwd(const srk_pixel_loss_args* a, srk_stream_t stream);
int srk_pixel_loss_bwd(const srk_pixel_loss_args* a, srk_stream_t stream);

/* PSNR loss (NAFNet's PSNRLoss on RGB): loss = (10 / ln 10) mean_n ln(mse_n + eps), mse_n the mean of d^2 over the `per` = C H W
 * elements of image n: minus the PSNR in dB.  Forward: block (n, b) of a grid that flattens (image, block) into ONE dimension (more
 * than 65,535 images work) writes the fp64 sum of d^2 over its share of image n into slot n * (blocks per image) + b.  An image starts
 * at element n * per of a 16-byte-aligned tensor, so its first (-n per) mod 4 elements and its last ones are read as scalars and the
 * float4 loads in between never hold another image's pixel.  Finalize: one workgroup, fixed order: mse_n, coef[n] = (10 / ln 10) / N
 * * 2 / (per (mse_n + eps)), the loss.  Backward: grad = ((*gout) * coef[n]) * d, 12 B per element.  An image equal to its target gives
 * ln(eps) and a zero gradient.  N * (blocks per image) < 2^24: a grid of fewer than 2^32 threads, which is what HIP launches. */
typedef struct srk_psnr_loss_args {
  const float* sr;                        /* [N][per] (forward, backward)                                                     */
  const float* hr;                        /* [N][per] (forward, backward)                                                     */
  int N;
  long long per;                          /* elements per image, C * H * W                                                    */
  float eps;
  double* partial;                        /* [srk_psnr_loss_blocks(N, per)]: per (image, block) sum of d^2                    */
  float* coef;                            /* [N]: finalize writes, backward reads                                             */
  float* loss;                            /* finalize: device scalar                                                          */
  const float* gout;                      /* backward: device scalar                                                          */
  float* grad;                            /* backward: [N][per] d loss / d sr                                                 */
} srk_psnr_loss_args;
/* blocks of the forward and the backward grid, N * (blocks per image), or -1 when the sizes are refused (N or per < 1, 2^24 blocks or more) */
long long srk_psnr_loss_blocks(int N, long long per);
int srk_psnr_loss_fwd(const srk_psnr_loss_args* a, srk_stream_t stream);
int srk_psnr_loss_finalize(const srk_psnr_loss_args* a, srk_stream_t stream);
int srk_psnr_loss_bwd(const srk_psnr_loss_args* a, srk_stream_t stream);

/* ---- frequency losses: the FFT loss (BasicSR's FFTLoss) and the focal frequency loss (Jiang et al., ICCV 2021), csrc/freq_loss.hip.
 * d = sr - hr, nothing clamped; per plane (n, c) of H x W the full unnormalised spectrum D[k][l] = sum_{h,w} d[h][w]
 * e^{-2 pi i (k h / H + l w / W)}.  At the self-conjugate bins (2k = 0 mod H and 2l = 0 mod W) Im D IS 0 (d is real): every kernel sets
 * it to 0 there and never keeps a rounding residue; its sign is 0 in the gradient.
 *   fft   L = (sum |Re D| + sum |Im D|) / (2 N C H W);  d L / d d = Re(F^H G) / (2 N C H W), G = sign(Re D) + i sign(Im D)
 *   ffl   q = |D|^2 / (H W), w = (q / q_max)^(alpha / 2) with q_max the plane's maximum, w a constant of the gradient;
 *         L = sum w q / (N C H W);  d L / d D = 2 w D / (H W) / (N C H W);  a plane with q_max = 0 gives loss 0 and gradient 0
 * The transform is a direct matrix DFT on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32: exact fp32).  d is real, so row H - k of the
 * spectrum is the conjugate of row k read backwards: only the rows k = 0 .. H / 2 are computed; the rows with 0 < 2k < H count twice, k = 0 and
 * (H even) k = H / 2 once.  The value is that of the full spectrum.
 * Twiddles: tw_h = [2][H] (cos, then sin, of 2 pi m / H, m = 0 .. H - 1; built in double, rounded to fp32 once), tw_w = [2][W]; the
 * kernels index them with (j k) mod n, formed with integers, and never call a sine or cosine.
 * Forward: one workgroup per (plane, block of 32 rows k): T = Fh[k block] d (32 x W complex, LDS; sr and hr are read here, once
 * per block), then D = T Fw per 32 columns in accumulators, the elementwise term on the accumulators, and per workgroup TWO doubles
 * in its own slot: (sum, max q) -- fft: sum of |Re D| + |Im D|, max unused (0); ffl: sum of q^(1 + alpha / 2), max of q.  The spectrum
 * never reaches memory.  Finalize: one workgroup, fixed order, double: per plane the sum of its blocks (ffl: over q_max^(alpha / 2),
 * and q_max to `qmax`), then the sum over planes and the division.  Backward, two launches: (1) the same workgroups recompute D, form
 * G in place (fft: the signs; ffl: 2 w D / (H W) with `qmax`), weight it by the row's count and apply the adjoint along the rows,
 * V = G Fw^H, written to `scratch`; (2) one workgroup per (plane, 32 columns): grad = Re(Fh^H V) * scale * (*gout), every element
 * written once.  No atomics, no host sync; hr gets no gradient.  NCHW fp32 contiguous, 1 <= H, W <= 512, 0 <= alpha <= 8 (beyond
 * that q^(1 + alpha / 2) leaves fp32 on images far outside [0, 1]: the caller computes in torch). */
#define SRK_FREQ_MAX_SIZE 512
#define SRK_FREQ_MAX_ALPHA 8
typedef struct srk_fft_loss_args {
  const float* sr;                        /* [N][C][H][W] (forward, backward)                                                  */
  const float* hr;                        /* [N][C][H][W] (forward, backward)                                                  */
  int N, C, H, W;
  const float* tw_h;                      /* [2][H]: cos, sin of 2 pi m / H                                                    */
  const float* tw_w;                      /* [2][W]: cos, sin of 2 pi m / W                                                    */
  double* partial;                        /* [srk_freq_loss_tiles(N, C, H, W)][2]: per workgroup (sum, 0)                      */
  float* loss;                            /* finalize: device scalar                                                           */
  float* scratch;                         /* backward: [N C][2][H / 2 + 1][W], written by its first launch, read by its second */
  const float* gout;                      /* backward: device scalar                                                           */
  float* grad;                            /* backward: [N][C][H][W] d loss / d sr                                              */
} srk_fft_loss_args;
typedef struct srk_ffl_loss_args {
  const float* sr;                        /* [N][C][H][W] (forward, backward)                                                  */
  const float* hr;                        /* [N][C][H][W] (forward, backward)                                                  */
  int N, C, H, W;
  float alpha;                            /* 0 <= alpha <= SRK_FREQ_MAX_ALPHA                                                  */
  const float* tw_h;                      /* [2][H]: cos, sin of 2 pi m / H                                                    */
  const float* tw_w;                      /* [2][W]: cos, sin of 2 pi m / W                                                    */
  double* partial;                        /* [srk_freq_loss_tiles(N, C, H, W)][2]: per workgroup (sum q^(1 + alpha / 2), max q) */
  float* qmax;                            /* [N C]: finalize writes each plane's largest q, backward reads                     */
  float* loss;                            /* finalize: device scalar                                                           */
  float* scratch;                         /* backward: [N C][2][H / 2 + 1][W], written by its first launch, read by its second */
  const float* gout;                      /* backward: device scalar                                                           */
  float* grad;                            /* backward: [N][C][H][W] d loss / d sr                                              */
} srk_ffl_loss_args;
/* workgroups of the forward over the whole batch, N C ceil((H / 2 + 1) / 32): the rows of `partial`; -1 when the sizes are refused */
int srk_freq_loss_tiles(int N, int C, int H, int W);
int srk_fft_loss_fwd(const srk_fft_loss_args* a, srk_stream_t stream);
int srk_fft_loss_finalize(const srk_fft_loss_args* a, srk_stream_t stream);
int srk_fft_loss_bwd(const srk_fft_loss_args* a, srk_stream_t stream);
int srk_ffl_loss_fwd(const srk_ffl_loss_args* a, srk_stream_t stream);
int srk_ffl_loss_finalize(const srk_ffl_loss_args* a, srk_stream_t stream);
int srk_ffl_loss_bwd(const srk_ffl_loss_args* a, srk_stream_t stream);

/* ---- SSIM with piq.ssim's defaults (reference srmodel.py:52-53,567-593 -> piq.ssim): images are average-pooled by
 * `pool` = max(1, round(min(H, W) / 256)) (floor division of the extent, as F.avg_pool2d), filtered with the separable
 * 11-tap Gaussian (sigma), and the SSIM map of the VALID region ((Hp-10) x (Wp-10)) is summed per (image, channel)
 * plane.  The caller divides by the map size and averages over channels and images.  Inputs are used as given
 * (the model clamps before its metrics).  fp32 NCHW planar. ------------------------------------------------------ */
typedef struct srk_ssim_args {
  const float* x;                         /* [N][C][H][W]                                                   */
  const float* y;
  int N, C, H, W;
  int pool;                               /* >= 1                                                           */
  float sigma, k1, k2;                    /* 1.5, 0.01, 0.03                                                */
  double* sums;                           /* [N*C] sums of the SSIM map, caller-zeroed                      */
} srk_ssim_args;
int srk_image_ssim(const srk_ssim_args* a, srk_stream_t stream);

/* ---- MS-SSIM with piq.multi_scale_ssim's defaults (reference configs/train_default_sr.yml `metrics`), csrc/ms_ssim.hip -----------
 * Five levels; level 0 is the input, level k > 0 is level k-1 replicate-padded by p = max(H % 2, W % 2) pixels on the top and
 * left only, then 2x2 / stride-2 average-pooled (floor).  No initial average-pool.  Per level and (image, channel) plane the SSIM
 * and contrast-structure maps (separable 11-tap Gaussian, sigma) are averaged over the valid region ((Hk-10) x (Wk-10));
 * v = prod_{k<4} relu(cs_k)^w_k * relu(ss_4)^w_4, and *out = the mean of v over channels and images.  H, W >= 161.
 * Inputs are used as given (the model clamps before its metrics).  fp32 NCHW planar.  No host sync, no float atomics.
 * workspace: srk_ms_ssim_workspace_bytes(N, C, H, W) bytes (levels 1-4 of both images);
 * partials: [N*C][srk_ms_ssim_tiles(H, W)][2] doubles, 16-byte aligned: per 16x16 map tile (sum ss, sum cs); the tiles of
 * level k of a plane are [first[k], first[k+1]).  ------------------------------------------------------------------------------ */
typedef struct srk_ms_ssim_args {
  const float* x;                         /* [N][C][H][W]                                                   */
  const float* y;
  float* workspace;
  double* partials;
  float* out;                             /* device scalar                                                  */
  int N, C, H, W;
  float sigma, k1, k2;                    /* 1.5, 0.01, 0.03                                                */
  float w0, w1, w2, w3, w4;               /* 0.0448, 0.2856, 0.3001, 0.2363, 0.1333                        */
} srk_ms_ssim_args;
/* bytes of the pyramid workspace (a multiple of 256), or -1 when the sizes are refused */
long long srk_ms_ssim_workspace_bytes(int N, int C, int H, int W);
/* map tiles per plane over all five levels (-1 when refused); first (nullable) receives the 6 level boundaries */
int srk_ms_ssim_tiles(int H, int W, int* first);
int srk_ms_ssim(const srk_ms_ssim_args* a, srk_stream_t stream);

/* ---- remaining conv models: SRResNet and DDBPN ---------------------------------------------------
 * im2col / col2im on NHWC tensors for any kernel size K, stride and zero padding:
 *   cols[n][oy][ox][(kh*K + kw)*C + c] = x[n][oy*stride + kh - pad][ox*stride + kw - pad][c]          (srk_unfold_nhwc)
 *   out[n][y][x][c] = bias[c] + sum of cols[n][iy][ix][(kh*K + kw)*C + c] over y = iy*stride - pad + kh, x = ...  (srk_fold_nhwc)
 * nn.Conv2d(k, stride, padding) (models/ddbpn.py:10-24 `projection_conv(up=False)`, the 9x9 tail conv of
 * models/srresnet.py:24-29) = srk_unfold_nhwc -> 1x1 srk_conv2d with the weight as a [Cout][K*K*Cin] matrix;
 * nn.ConvTranspose2d (ddbpn.py `projection_conv(up=True)`) = 1x1 srk_conv2d to K*K*Cout channels -> srk_fold_nhwc.
 * Each kernel is the other's adjoint, so the data gradients use the same pair.                                   */
typedef struct {
  const void* x; int x_pitch, x_coff;     /* NHWC input, C channels from x_coff                                   */
  void* cols; int cols_pitch;             /* out [N][Ho][Wo][>= K*K*C]                                             */
  int N, H, W, C;                         /* C: multiple of 16 bytes / sizeof(dtype)                               */
  int K, stride, pad;
  int Ho, Wo;                             /* (H + 2 pad - K) / stride + 1                                           */
  int dtype;
} srk_unfold_nhwc_args;
int srk_unfold_nhwc(const srk_unfold_nhwc_args* a, srk_stream_t stream);

typedef struct {
  const void* cols; int cols_pitch;       /* [N][Hi][Wi][>= K*K*C]                                                  */
  const float* bias;                      /* [C] added once per output element, or NULL                             */
  void* out; int out_pitch, out_coff;     /* NHWC [N][Ho][Wo][C]                                                    */
  int N, Hi, Wi, C;
  int K, stride, pad;
  int Ho, Wo;                             /* ConvTranspose2d: (Hi - 1)*stride - 2 pad + K                           */
  int dtype;
} srk_fold_nhwc_args;
int srk_fold_nhwc(const srk_fold_nhwc_args* a, srk_stream_t stream);

/* D-DBPN's projection convolutions at scale 4, directly (csrc/proj.hip): nn.Conv2d / nn.ConvTranspose2d(32, 32, kernel 8, stride 4,
 * padding 2) -- /root/reference models/ddbpn.py:10-24 `projection_conv` as `DenseProjection` uses it (ddbpn.py:42-53) -- on NHWC
 * 16-bit tensors, no column tensor.  Replaces the cuDNN strided / transposed convolutions behind those modules and their autograd.
 * One weight convention for both module kinds: w4[cl][ch][ky][kx], cl = channel on the LOW-resolution side, ch = channel on the
 * HIGH-resolution side (Conv2d's [out][in][ky][kx], ConvTranspose2d's [in][out][ky][kx]).  (N, H, W) are the LOW-resolution dims;
 * the other tensor is [N][4H][4W].
 *   srk_proj_down : HR -> LR   out[q][cl] = bias[cl] + sum xh[4q - 2 + k][ch] w4[cl][ch][k]     (Conv2d forward; ConvTranspose2d dgrad)
 *   srk_proj_up   : LR -> HR   out[4q - 2 + k][ch] += x[q][cl] w4[cl][ch][k], + bias[ch]         (ConvTranspose2d forward; Conv2d dgrad)
 *   srk_proj_wgrad: dw4[cl][ch][k] (=, +=) sum_q g[q][cl] xh[4q - 2 + k][ch]                     ((xh, g) = (x, dy) resp. (dy, x))
 * srk_proj_pack turns fp32 w4 into the MFMA fragment order of both directions: wpk (srk_proj_pack_bytes() bytes, 16-byte aligned)
 * holds the `down` fragments first, the `up` fragments at byte srk_proj_pack_bytes() / 2.                                     */
typedef struct {
  const void* x; int x_pitch;             /* input NHWC, 32 channels used, pitch in elements                                */
  void* out; int out_pitch;
  const void* wpk;                        /* the direction's half of srk_proj_pack's output                                 */
  const float* bias;                      /* [32] or NULL                                                                   */
  int N, H, W;                            /* low-resolution dims                                                            */
  int dtype;                              /* SRK_BF16 / SRK_F16                                                             */
  const float* slope; int slope_stride;   /* fused nn.PReLU (ddbpn.py:42-53: every projection conv is followed by one), or NULL: */
  void* pre; int pre_pitch;               /* out = prelu(stored conv output), pre (or NULL) = the stored conv output, for its backward */
} srk_proj_args;
long long srk_proj_pack_bytes(void);
int srk_proj_pack(const float* w4, void* wpk, int dtype, srk_stream_t stream);
/* the same for n (weights, packed buffer) pairs in ONE launch: `table_dev` is a device array (D-DBPN: its 33 projections per step) */
typedef struct { const float* w4; void* wpk; } srk_proj_pack_job;
int srk_proj_pack_group(const srk_proj_pack_job* table_dev, int n, int dtype, srk_stream_t stream);
int srk_proj_down(const srk_proj_args* a, srk_stream_t stream);
int srk_proj_up(const srk_proj_args* a, srk_stream_t stream);
typedef struct {
  const void* xh; int xh_pitch;           /* high-resolution operand [N][4H][4W][>= 32]                                     */
  const void* g; int g_pitch;             /* low-resolution operand [N][H][W][>= 32]                                        */
  float* scratch;                         /* srk_proj_wgrad_scratch_floats(N, H, W) floats                                  */
  float* dw;                              /* [32][32][8][8] fp32                                                            */
  int accumulate;                         /* 1: dw += (an existing gradient)                                                */
  int N, H, W;
  int dtype;
  float* db;                              /* bias gradient [32] (sum of the upstream gradient over its pixels), or NULL     */
  int bias_side;                          /* which operand is the upstream gradient: 1 = g (Conv2d), 2 = xh (ConvTranspose2d) */
  int db_accumulate;
} srk_proj_wgrad_args;
long long srk_proj_wgrad_scratch_floats(int N, int H, int W);
int srk_proj_wgrad(const srk_proj_wgrad_args* a, srk_stream_t stream);

/* Per-channel partial sums over P pixels of an NHWC tensor (fp32 accumulate), one plain store per block and channel:
 * partial[b][0][c], partial[b][1][c] for b < srk_chan_stats_blocks(P); the caller adds the blocks in order.
 *   mode 0: sum x, sum x^2          nn.BatchNorm2d batch statistics (srresnet.py:16-21 via common.py:97-98) in ONE pass over
 *                                   values shifted by the tensor's first pixel (shift_out != NULL), or one pass for the mean
 *                                   and a second pass with shift = mean for the variance
 *   mode 1: sum y, sum x*y          BatchNorm backward (y = upstream gradient)
 *   mode 2: sum over x <= 0 of x*y  nn.PReLU slope gradient (partial[b][1] = 0)                                   */
typedef struct {
  const void* x; int x_pitch, x_coff;
  const void* y; int y_pitch, y_coff;     /* modes 1, 2                                                             */
  long long P; int C;                     /* C <= 256                                                               */
  int mode;
  float* partial;                         /* [blocks][2][C]                                                         */
  int dtype;
  const float* shift;                     /* [C] or NULL: x is replaced by x - shift[c] in every sum (second pass of a  */
                                          /* two-pass variance, centred BatchNorm backward: no cancellation in fp32)   */
  float* shift_out;                       /* [C] or NULL (then `shift` must be NULL): shift[c] = x[pixel 0][c], also    */
                                          /* stored here -- the shifted-data variance: E[(x-K)^2] - (E[x-K])^2 with K a */
                                          /* value of the data loses no digits to |mean| >> std                         */
  void* gate_out; int gate_pitch;         /* mode 2 only, or NULL: gate_out[p][c] = y * (x > 0 ? 1 : slope[c]) -- nn.PReLU's */
  const float* slope; int slope_stride;   /* input gradient written by the pass that sums its slope gradient (one read of x, y) */
  /* mode 3: nn.BatchNorm2d's backward BEHIND an nn.PReLU (srresnet.py:16-21) in one pass: x = the BatchNorm's input, y = the gradient
   * of the PReLU's output; with yb = gate_a x + gate_d (the BatchNorm's output, recomputed) and gp = y (yb > 0 ? 1 : slope):
   * partial[b][0] = sum gp, partial[b][1] = sum (x - shift) gp, partial2[b] = sum over yb <= 0 of yb y (the slope's gradient)   */
  const float* gate_a; const float* gate_d;   /* [C] fp32: the forward scale / shift (srk_chan_finalize mode 1, rows 2 and 3)   */
  float* partial2;                        /* [blocks][C]                                                                    */
} srk_chan_stats_args;
int srk_chan_stats_blocks(long long P);
int srk_chan_stats(const srk_chan_stats_args* a, srk_stream_t stream);
/* The per-channel step between srk_chan_stats and srk_chan_apply of nn.BatchNorm2d (models/common.py:97-98 in srresnet.py:16-21)
 * and nn.PReLU, as one launch: the ordered sum over the blocks of `partial` [nblocks][2][C] and the vector arithmetic.
 *   mode 0: out[0] = mean = sum0 / M
 *   mode 1 (sums of x - K, K = `mean`: the mean of a first pass, or srk_chan_stats' shift_out): the batch mean = K + sum0/M
 *           (out row 4), var = max(sum1/M - (sum0/M)^2, 0); running_mean / running_var (nullable, [Creal]) updated with
 *           `momentum` (unbiased variance, like torch); out rows: invstd = rsqrt(var + eps), gamma (weight padded with 0),
 *           a = gamma * invstd, d = beta - mean * a, mean  (srk_chan_apply: out = a x + d)
 *   mode 2 (sum0 = sum dy, sum1 = sum (x - mean) dy; batch statistics): out rows: dgamma = invstd sum1, dbeta = sum0,
 *           a = gamma invstd, b = -a invstd dgamma / M, d = -a dbeta / M - b mean     (dx = a dy + b x + d)
 *   mode 3 (running statistics): out rows: dgamma, dbeta, a = gamma invstd
 *   mode 4: out[0][c] = sum0 (PReLU slope gradients); total = 1: one number, summed over the channels too; `dgamma_acc`
 *           (nullable, [Creal] or [1]): the slope's existing .grad buffer, += the result                               */
typedef struct {
  const float* partial; int nblocks; int C; int Creal;
  int mode; int total;
  float M, eps, momentum;
  const float* mean; const float* invstd; const float* gamma;
  const float* weight; const float* bias;
  float* running_mean; float* running_var;
  float* out;                             /* [rows][C] fp32 */
  long long* nbt;                         /* mode 1, nullable: nn.BatchNorm2d.num_batches_tracked, += 1                          */
  float* dgamma_acc; float* dbeta_acc;    /* modes 2 / 3, nullable, [Creal]: the parameters' existing .grad buffers, += dgamma / dbeta */
  const float* partial2; int total2;      /* modes 2 / 3, nullable: srk_chan_stats mode 3's third sums [nblocks][C] -> out row 5 = the  */
  float* dslope_acc;                      /* PReLU slope gradient (total2: ONE number, summed over the channels); += into dslope_acc    */
} srk_chan_finalize_args;
int srk_chan_finalize(const srk_chan_finalize_args* a, srk_stream_t stream);
/* srk_chan_stats and srk_chan_finalize as ONE launch: the block that finishes last does the finalize step.  `f->partial` and
 * `f->nblocks` are taken from `a`; `counter`: one int in device memory, 0 before the first use (the kernel leaves it 0) and not shared
 * by launches that may run at the same time.                                                                          */
int srk_chan_stats_finalize(const srk_chan_stats_args* a, const srk_chan_finalize_args* f, int* counter, srk_stream_t stream);

/* out[p][c] = post( (a[c]*x + b[c]*y + d[c]) * gate ),  gate = (z > 0 ? 1 : slope[c*slope_stride]) when z is given,
 * post = PReLU with the same slope when post_prelu.  a / b / d NULL = 1 / 1 / 0; y NULL = no second input.
 * BatchNorm apply (+ residual in y), BatchNorm backward (x = dy, y = saved input), nn.PReLU forward and backward.  */
typedef struct {
  const void* x; int x_pitch, x_coff;
  const void* y; int y_pitch, y_coff;
  const void* z; int z_pitch, z_coff;
  const float* a; const float* b; const float* d;   /* [C] fp32                                                     */
  const float* slope; int slope_stride;    /* nn.PReLU weight: stride 1 = per channel, 0 = one shared value           */
  int post_prelu;
  void* out; int out_pitch, out_coff;
  long long P; int C;
  int dtype;
  const float* gate_a; const float* gate_d;   /* [C] or NULL.  Given (with z and slope): the gate's argument is gate_a z + gate_d and   */
                                              /* only the first term passes it: out = a x gate + b y + d (BatchNorm backward behind a  */
                                              /* PReLU: x = dy, y = z = the BatchNorm's input)                                          */
} srk_chan_apply_args;
int srk_chan_apply(const srk_chan_apply_args* a, srk_stream_t stream);

/* ---- the last upsampling stage and the tail conv as ONE linear map (csrc/hr_tail.hip) ----------------------------------------
 * Replaces, on the 16-bit path, the end of EDSR / RCAN / RDN: UpscaleBlock's last `conv3x3(Ci -> 4C) -> nn.PixelShuffle(2)` stage
 * (models/common.py:112-139, no activation on this path) followed by the tail `conv3x3(C -> O)` (edsr.py:37-38,49-52, rcan.py:83-87,
 * 102-104, rdn.py:85-95), and their autograd.  Two convolutions with nothing non-linear between them are one linear map of the
 * upsampler's input X: at X's resolution, with the 4 sub-pixel positions (a, b) of an output pixel as channels k = o*4 + a*2 + b,
 *     T[(2y+a, 2x+b)][o] = beff[k] + sum_{ci, f in [-2,2]^2} weff[k][ci][f] X[(y,x) + f][ci]  -  (border terms on the outermost ring)
 * a 5x5 convolution Ci -> 4O (srk_conv2d / srk_conv2d_wgrad: the direct large-kernel kernels) whose weights are sums of products
 * Wt Wu.  The C-channel tensor at the doubled resolution (1.2 GB at EDSR-baseline's batch of 256) and its gradient never exist.
 * The border terms make the result EXACT: the tail conv pads the shuffled tensor with zeros, so output pixels of the outermost ring
 * lose the taps that leave the image; those terms are linear in X too (one row / column of 5 taps per edge, one tap per corner).
 *   srk_hrtail_collapse   : (wt, bt, wu, bu) -> weff, beff, wedge, bedge, wcor, bcor                          (parameter-sized)
 *   srk_hrtail_edge_fwd   : out -= border terms (out: what srk_conv2d wrote with weff, planar fp32 + PixelShuffle(2))
 *   srk_hrtail_edge_bwd_x : dx -= (border terms)^T g    (dx: what the data-gradient srk_conv2d wrote)
 *   srk_hrtail_edge_bwd_w : correlations of g and x over the edge rows / columns / corner pixels -> eedge, e0, ecor, k0
 *   srk_hrtail_expand     : (r = dL/dweff, r0 = dL/dbeff from srk_conv2d_wgrad; eedge ...) -> dwt, dbt, dwu, dbu  (parameter-sized)
 * Layouts (fp32): weff [4O][Ci][5][5]; wedge / eedge [4][2O][Ci][5] and bedge / e0 [4][2O]: edge 0 top, 1 bottom (row kk = o*2 + b, 5
 * taps along x), 2 left, 3 right (kk = o*2 + a, 5 taps along y); wcor / ecor [4][O][Ci] and bcor / k0 [4][O]: corner a*2 + b.
 * wu's output channels are in torch's PixelShuffle order c*4 + i*2 + j.  O <= 4.                                            */
typedef struct {
  const float* wt; const float* bt;     /* tail conv [O][C][3][3], [O] or NULL                                    */
  const float* wu; const float* bu;     /* upsampler conv [4C][Ci][3][3], [4C] or NULL                            */
  int O, C, Ci;
  float* weff; float* beff;             /* collapse: out; the launches in between: srk_pack_conv_weights' input   */
  float* wedge; float* bedge; float* wcor; float* bcor;
  const void* x; int x_pitch;           /* NHWC 16-bit [N][H][W][>= Ci]                                           */
  int N, H, W; int dtype;
  float* out;                           /* edge_fwd: [N][O][2H][2W] fp32, corrected in place                      */
  const float* g;                       /* edge_bwd_*: gradient of out, [N][O][2H][2W] fp32                       */
  void* dx; int dx_pitch;               /* edge_bwd_x: NHWC 16-bit [N][H][W][>= Ci], corrected in place           */
  float* eedge; float* e0; float* ecor; float* k0;   /* edge_bwd_w: out; expand: in                               */
  float* scratch;                       /* edge_bwd_w: srk_hrtail_scratch_floats(N, Ci) floats                    */
  const float* r; const float* r0;      /* expand: dL/dweff [4O][Ci][5][5], dL/dbeff [4O]                         */
  float* dwt; float* dbt; float* dwu; float* dbu;    /* expand: out (dbt / dbu nullable)                          */
} srk_hrtail_args;
int srk_hrtail_collapse(const srk_hrtail_args* a, srk_stream_t stream);
int srk_hrtail_edge_fwd(const srk_hrtail_args* a, srk_stream_t stream);
int srk_hrtail_edge_bwd_x(const srk_hrtail_args* a, srk_stream_t stream);
long long srk_hrtail_scratch_floats(int N, int Ci);
int srk_hrtail_edge_bwd_w(const srk_hrtail_args* a, srk_stream_t stream);
int srk_hrtail_expand(const srk_hrtail_args* a, srk_stream_t stream);

/* ---- optimizer: Adam over every parameter tensor in one launch -----------------------------------
 * Replaces torch.optim.Adam(...).step() as models/srmodel.py:145-154 configures it (torch defaults; :602-603 drops every
 * user-supplied hyper-parameter).  fp32 parameters, gradients and moments.  The tensors are described by a DEVICE table
 * (srk_adam_slot), the work by a device list of blocks (srk_adam_block: `count` elements of tensor `slot` from `start`);
 * the first and second moments of all tensors live in two flat buffers `m` / `v`, tensor i at `state_off` floats.
 *     t = steps[step_idx] + 1;  g' = maximize ? -g : g;  g' += weight_decay * p;
 *     m += (g' - m) * (1 - beta1);  v = beta2 * v + (1 - beta2) * g' * g';
 *     p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * `steps` (device floats: the number of updates each tensor has had -- torch counts per parameter, a tensor without a
 * gradient skips the step) are advanced by the call itself (a second tiny launch) for the tensors in the table, so a
 * captured hipGraph can replay it; `ticket` is reserved (may be NULL).
 * `lr_dev` (this struct and the three optimizers' below): NULL, or the address of ONE DEVICE double that every entry point of the
 * family reads when the launch RUNS -- a replayed hipGraph follows a learning rate that srk_lr_sched_step (or an upload) wrote
 * between two replays.  The value is rounded exactly where the by-value `lr` is: (float)lr here, (float)(-s*lr), (float)(-wd*lr),
 * (float)(-lr) below.  With `lr_dev` the by-value `lr` is neither read nor range-checked.                                  */
typedef struct { float* p; const float* g; long long state_off; long long n; long long step_idx; } srk_adam_slot;
typedef struct { int slot; int count; long long start; } srk_adam_block;
typedef struct {
  const srk_adam_slot* slots; const srk_adam_block* blocks; int nslots, nblocks;
  float* m; float* v;
  float* steps; unsigned int* ticket;
  float lr, beta1, beta2, eps, weight_decay; int maximize;
  float one_minus_beta1, one_minus_beta2;   /* 1 - beta rounded from double, as torch forms them */
  const double* lr_dev;                     /* NULL: `lr` above.  Else ONE DEVICE double read when the launch RUNS (srk_lr_sched_step) */
} srk_adam_args;
int srk_adam_step(const srk_adam_args* a, srk_stream_t stream);
/* The same update under DYNAMIC LOSS SCALING kept on the device (fp16 training: the reference's `precision: 16` runs Lightning's
 * "16-mixed" = autocast + torch.amp.GradScaler, configs/all.yml:122; GradScaler decides on the HOST whether to call
 * optimizer.step, which a hipGraph replay cannot do).  scaler_state: 8 device floats {scale, growth tracker, found_inf, growth
 * factor, backoff factor, growth interval, skipped steps, reserved}.  The gradients in the table are still multiplied by `scale`:
 *   srk_adam_step_scaled : found_inf |= any gradient not finite; if not found_inf: the update on g / scale, step counts += 1
 *                          (a step with a non-finite gradient changes NOTHING, like GradScaler.step)
 *   srk_loss_scale_update: once per step behind the last parameter group: found_inf ? scale *= backoff, tracker = 0
 *                          : (++tracker == interval ? scale *= growth, tracker = 0);  found_inf = 0     (GradScaler.update)      */
int srk_adam_step_scaled(const srk_adam_args* a, float* scaler_state, srk_stream_t stream);
/* the two halves of srk_adam_step_scaled for optimizers with SEVERAL parameter groups: GradScaler.step checks every group's
 * gradients before it updates any (torch/amp/grad_scaler.py: `found_inf` over all groups, then optimizer.step or nothing), so
 * call srk_adam_check_scaled for every group first, then srk_adam_update_scaled for every group, then srk_loss_scale_update */
int srk_adam_check_scaled(const srk_adam_args* a, float* scaler_state, srk_stream_t stream);
int srk_adam_update_scaled(const srk_adam_args* a, const float* scaler_state, srk_stream_t stream);
int srk_loss_scale_update(float* scaler_state, srk_stream_t stream);

/* ---- optimizer: Ranger (torch_optimizer 0.3.0 `Ranger`: RAdam + Lookahead) over the same table ---------------------------
 * The models' `optimizer="Ranger"` (reference models/srmodel.py:57-64).  The tensors and blocks are srk_adam_slot / srk_adam_block;
 * `m`, `v`, `slow` are the flat exp_avg / exp_avg_sq / slow_buffer of all tensors (tensor i at `state_off`).  Per tensor:
 *     t = steps[step_idx] + 1;  v = b2*v + (1-b2)*g*g;  m = b1*m + (1-b1)*g;
 *     N_max = 2/(1-b2) - 1;  b2t = b2^t;  N = N_max - 2*t*b2t/(1-b2t)
 *     s = N > n_sma_threshold ? sqrt((1-b2t)*(N-4)/(N_max-4)*(N-2)/N*N_max/(N_max-2)) / (1-b1^t) : 1/(1-b1^t)
 *     p += (-weight_decay*lr) * p   (weight_decay != 0);   p += (-s*lr) * (N > thr ? m/(sqrt(v)+eps) : m)
 *     t == 1: slow = p (before the update);   t % k == 0: slow += alpha*(p - slow); p = slow
 * N and s are computed in DOUBLE from the double hyper-parameters below (N cancels catastrophically at small t); -s*lr and
 * -weight_decay*lr are rounded to fp32 once; the element arithmetic is fp32.  Step counts advance as srk_adam_step's do.
 * srk_ranger_step_scaled / _check_scaled / _update_scaled: srk_adam_*'s loss-scaling contract (then srk_loss_scale_update). */
typedef struct {
  const srk_adam_slot* slots; const srk_adam_block* blocks; int nslots, nblocks;
  float* m; float* v; float* slow;
  float* steps;
  double lr, beta1, beta2, alpha, n_sma_threshold, eps, weight_decay;
  int k;
  const double* lr_dev;                     /* NULL: `lr` above; else as srk_adam_args.lr_dev */
} srk_ranger_args;
int srk_ranger_step(const srk_ranger_args* a, srk_stream_t stream);
int srk_ranger_step_scaled(const srk_ranger_args* a, float* scaler_state, srk_stream_t stream);
int srk_ranger_check_scaled(const srk_ranger_args* a, float* scaler_state, srk_stream_t stream);
int srk_ranger_update_scaled(const srk_ranger_args* a, const float* scaler_state, srk_stream_t stream);

/* ---- optimizer: SGD (torch.optim.SGD) over the same table -------------------------------------------------------------------
 * The models' `optimizer="SGD"` (reference models/srmodel.py:57-64).  The tensors and blocks are srk_adam_slot / srk_adam_block;
 * `buf` is the flat momentum_buffer of all tensors (tensor i at `state_off`; NULL iff momentum == 0).  Per tensor:
 *     g' = maximize ? -g : g;   g' += weight_decay * p                        (weight_decay != 0)
 *     momentum != 0:  buf = steps[step_idx] == 0 ? g' : momentum * buf + (1 - dampening) * g'
 *                     g' = nesterov ? g' + momentum * buf : buf
 *     p += (-lr) * g'
 * "first" (steps[step_idx] == 0) is torch's `momentum_buffer is None`: the buffer starts as a copy of the first gradient the
 * tensor ever receives, whatever `dampening` is.  It is read from the DEVICE count, which the call itself advances (a second
 * tiny launch) for the tensors in the table: a tensor without a gradient is not in the table and stays "first", and a replayed
 * hipGraph takes the branch of the step it replays.  momentum == 0: neither `buf` nor `steps` is read or written (both may be NULL).
 * -lr and 1 - dampening are formed in double and rounded to fp32 once; the element arithmetic is fp32 in torch's order.
 * Traffic: 12 B per parameter (p read + written, g read); 20 B with momentum (16 B at a tensor's first step: buf is only written).
 * srk_sgd_step_scaled / _check_scaled / _update_scaled: srk_adam_*'s loss-scaling contract (a step with a non-finite gradient changes
 * nothing, the counts and so the "first" flags included; then srk_loss_scale_update). */
typedef struct {
  const srk_adam_slot* slots; const srk_adam_block* blocks; int nslots, nblocks;
  float* buf;
  float* steps;
  double lr, momentum, dampening, weight_decay;
  int nesterov, maximize;
  const double* lr_dev;                     /* NULL: `lr` above; else as srk_adam_args.lr_dev */
} srk_sgd_args;
int srk_sgd_step(const srk_sgd_args* a, srk_stream_t stream);
int srk_sgd_step_scaled(const srk_sgd_args* a, float* scaler_state, srk_stream_t stream);
int srk_sgd_check_scaled(const srk_sgd_args* a, float* scaler_state, srk_stream_t stream);
int srk_sgd_update_scaled(const srk_sgd_args* a, const float* scaler_state, srk_stream_t stream);

/* ---- optimizer: RMSprop (torch.optim.RMSprop) over the same table -----------------------------------------------------------
 * The models' `optimizer="RMSprop"`.  `sq`, `buf`, `ga` are the flat square_avg, momentum_buffer (NULL iff momentum == 0) and
 * grad_avg (NULL iff !centered) of all tensors.  Per tensor, with g' as for SGD:
 *     sq = alpha * sq + (1 - alpha) * g' * g'
 *     centered:  ga += (g' - ga) * (1 - alpha);  avg = sqrt(sq - ga * ga) + eps          else  avg = sqrt(sq) + eps
 *     momentum > 0:  buf = momentum * buf + g' / avg;  p += (-lr) * buf                  else  p += (-lr) * (g' / avg)
 * Only the buffers the configuration uses are touched: 20 B per parameter plain, +8 B with momentum, +8 B centered.  Scalars as
 * for SGD; `steps` (torch's per-parameter `step`) advance as srk_adam_step's do.  _step_scaled / _check_scaled / _update_scaled:
 * srk_adam_*'s loss-scaling contract (then srk_loss_scale_update). */
typedef struct {
  const srk_adam_slot* slots; const srk_adam_block* blocks; int nslots, nblocks;
  float* sq; float* buf; float* ga;
  float* steps;
  double lr, alpha, eps, weight_decay, momentum;
  int centered, maximize;
  const double* lr_dev;                     /* NULL: `lr` above; else as srk_adam_args.lr_dev */
} srk_rmsprop_args;
int srk_rmsprop_step(const srk_rmsprop_args* a, srk_stream_t stream);
int srk_rmsprop_step_scaled(const srk_rmsprop_args* a, float* scaler_state, srk_stream_t stream);
int srk_rmsprop_check_scaled(const srk_rmsprop_args* a, float* scaler_state, srk_stream_t stream);
int srk_rmsprop_update_scaled(const srk_rmsprop_args* a, const float* scaler_state, srk_stream_t stream);

/* ---- exponential moving average of the weights (ema.py), csrc/ema.hip ----------------------------------------------------------
 * One launch over the optimizers' table: srk_adam_slot (`p` the parameter, `g` unused and NULL, `state_off` the tensor's offset in
 * floats into the flat fp32 `shadow` buffer, `step_idx` unused) and srk_adam_block (one tensor per block).  `op`:
 *     SRK_EMA_UPDATE : s = s + w * (p - s),  w = weight[0];  count[0] += 1 (one thread, an ordinary store)
 *     SRK_EMA_SWAP   : p and s exchanged element by element (two swaps restore every bit)
 *     SRK_EMA_STORE  : s = p            SRK_EMA_LOAD : p = s
 * `weight` is ONE DEVICE float, w = (float)(1.0 - decay) formed in double by the host, and `count` ONE DEVICE 64-bit integer: both are
 * read when the launch RUNS, so a replayed hipGraph counts its updates and follows a decay written between two replays.  UPDATE is
 * at::lerp's form for w < 0.5 (torch.optim.swa_utils.get_ema_multi_avg_fn) used for EVERY w: fp32, three roundings, not contracted.
 * One exception: w == 1 (decay 0) stores p itself -- the formula's exact value, which fp32's s + (p - s) can miss by an ulp.
 * `weight` and `count` may be NULL for the other three operations.  Traffic: 12 B per parameter (UPDATE), 16 B (SWAP), 8 B. */
enum { SRK_EMA_UPDATE = 0, SRK_EMA_SWAP = 1, SRK_EMA_STORE = 2, SRK_EMA_LOAD = 3 };
typedef struct {
  const srk_adam_slot* slots; const srk_adam_block* blocks; int nslots, nblocks;
  float* shadow;
  const float* weight;
  long long* count;
  int op;
} srk_ema_args;
int srk_ema_step(const srk_ema_args* a, srk_stream_t stream);

/* ---- learning-rate schedules on the device (lr_sched.py), csrc/lr_sched.hip ------------------------------------------------------
 * One tiny launch that keeps a schedule's step count and the learning rate of every parameter group in DEVICE memory, where the
 * optimizers' `lr_dev` reads them: a captured step that ends in SRK_LR_ADVANCE follows the schedule replay after replay.
 *   count   : ONE device 64-bit integer, the number of optimizer steps so far (t)
 *   lr      : device double [ngroups], written:  lr[g] = f(t, base_lr[g])
 *   base_lr : device double [ngroups], read
 *   op      : SRK_LR_SET      count = value;  lr = f(count)        (creation, load_state_dict)
 *             SRK_LR_ADVANCE  count += 1;     lr = f(count)        (behind every optimizer step)
 * f(t, base) = warm(t) * main(t, base), in DOUBLE, torch.optim.lr_scheduler's closed forms:
 *   warm  : 1 if warmup_steps == 0, else warmup_start + (1 - warmup_start) * min(t, W) / W          LinearLR(warmup_start, 1, W)
 *   SRK_LR_CONSTANT        : base
 *   SRK_LR_STEP            : base * gamma^(t / step_size)  (integer division)                        StepLR
 *   SRK_LR_MULTISTEP       : base * gamma^(number of milestones <= t)                                MultiStepLR
 *   SRK_LR_COSINE          : eta_min + (base - eta_min) * (1 + cos(pi * t / t_max)) / 2              CosineAnnealingLR (periodic past t_max)
 *   SRK_LR_COSINE_RESTARTS : the same in T_cur / T_i, found by the integer loop
 *                            T_cur = t, T_i = t_0;  while (T_cur >= T_i) { T_cur -= T_i; T_i *= t_mult; }   CosineAnnealingWarmRestarts
 * Only the constants of `kind` (and the warm-up's) are read and checked: step_size >= 1, t_max >= 1, t_0 >= 1, t_mult >= 1, at most
 * SRK_LR_MAX_MILESTONES milestones m0 <= m1 <= ... (the first `nmilestones` of m0..m15); always: 0 < warmup_start <= 1 (1 without a
 * warm-up), warmup_steps >= 0, value >= 0 for SRK_LR_SET.  One workgroup, one thread per group, ordinary stores. */
enum { SRK_LR_CONSTANT = 0, SRK_LR_STEP = 1, SRK_LR_MULTISTEP = 2, SRK_LR_COSINE = 3, SRK_LR_COSINE_RESTARTS = 4 };
enum { SRK_LR_SET = 0, SRK_LR_ADVANCE = 1 };
#define SRK_LR_MAX_MILESTONES 16
typedef struct {
  long long* count; double* lr; const double* base_lr; int ngroups;
  int kind, op;
  long long value;
  long long step_size; double gamma;
  int nmilestones;
  long long m0, m1, m2, m3, m4, m5, m6, m7, m8, m9, m10, m11, m12, m13, m14, m15;
  long long t_max; double eta_min;
  long long t_0, t_mult;
  long long warmup_steps; double warmup_start;
} srk_lr_sched_args;
int srk_lr_sched_step(const srk_lr_sched_args* a, srk_stream_t stream);

/* ---- gradient clipping by norm and by value (grad_clip.py), csrc/grad_clip.hip ------------------------------------------------------
 * torch.nn.utils.clip_grad_norm_ (norm_type 2) / clip_grad_value_ over the optimizers' table (srk_adam_slot: `g` the fp32 gradient,
 * clipped IN PLACE; `p`, `state_off`, `step_idx` unused; srk_adam_block: one workgroup per block), as launches of the step itself.
 * `state`: SRK_CLIP_STATE_FLOATS device floats, indexed by SRK_CLIP_*:
 *     MAX_NORM, CLIP_VALUE : the thresholds, read when a launch RUNS (a replayed hipGraph follows a value written between two replays)
 *     TOTAL_NORM, COEF     : what the last srk_grad_clip_coef computed
 *     NUM_CLIPPED, NUM_NONFINITE : how many of its runs had coef < 1 / a norm that was not finite (floats: exact up to 2^24)
 * `partials`: device doubles, one per block of EVERY parameter group's table; `base`: the first entry of this launch's group.
 * `scaler_state`: NULL, or optim.DeviceGradScaler's device floats when the gradients still carry the loss scale s = scaler_state[0].
 *   srk_grad_sumsq      (per group)  partials[base + b] = sum of g*g over block b: every element squared and added in double, thread by
 *                        thread in one fixed element order (the same for aligned and unaligned gradients), the 256 thread sums
 *                        combined in a fixed order.  No atomics, nothing to zero: the same gradients give the same bits.
 *   srk_grad_clip_coef  (once)  sum = partials[0] + ... + partials[nblocks_total - 1] in double, fixed order;  norm = sqrt(sum) / s;
 *                        coef = min(1, max_norm / (norm + 1e-6)) in double (torch's formula);  TOTAL_NORM = (float)norm,
 *                        COEF = (float)coef;  NUM_CLIPPED += 1 if (float)coef < 1.  A norm that is not finite: COEF = 1,
 *                        NUM_NONFINITE += 1 -- the gradients pass on unchanged (the loss scaler skips the step, or the optimizer sees them).
 *   srk_grad_clip_apply (per group)  g *= COEF in fp32.  A workgroup that reads COEF == 1 returns before it touches the gradient.
 *   srk_grad_clip_value (per group)  g = g < -b ? -b : (g > b ? b : g),  b = CLIP_VALUE, or (float)(CLIP_VALUE * s) in fp32 under the
 *                        scaler; a NaN stays a NaN (torch.clamp), and under the scaler an infinite g stays infinite, so that the
 *                        scaler's check behind this launch still finds both and skips the step (GradScaler.unscale_ records an
 *                        overflow BEFORE torch's clip); without a scaler +-inf becomes +-b, as torch.clamp gives.
 * Traffic per parameter: sumsq 4 B, apply 8 B (0 B when nothing is clipped), value 8 B. */
enum { SRK_CLIP_MAX_NORM = 0, SRK_CLIP_CLIP_VALUE = 1, SRK_CLIP_TOTAL_NORM = 2, SRK_CLIP_COEF = 3, SRK_CLIP_NUM_CLIPPED = 4,
       SRK_CLIP_NUM_NONFINITE = 5 };
#define SRK_CLIP_STATE_FLOATS 8
typedef struct {
  const srk_adam_slot* slots; const srk_adam_block* blocks; int nslots, nblocks;   /* sumsq, apply, value: this group's table */
  float* state;
  double* partials;                         /* sumsq: written; coef: read                                      */
  int base;                                 /* sumsq: this group's first entry of `partials`                    */
  int nblocks_total;                        /* coef: entries of `partials` (the blocks of all groups)           */
  const float* scaler_state;                /* coef, value: NULL, or the loss scaler's state (s = scaler_state[0]) */
} srk_grad_clip_args;
int srk_grad_sumsq(const srk_grad_clip_args* a, srk_stream_t stream);
int srk_grad_clip_coef(const srk_grad_clip_args* a, srk_stream_t stream);
int srk_grad_clip_apply(const srk_grad_clip_args* a, srk_stream_t stream);
int srk_grad_clip_value(const srk_grad_clip_args* a, srk_stream_t stream);

/* ---- gradient accumulation over micro-batches (grad_accum.py), csrc/grad_accum.hip ------------------------------------------------
 * One launch over the optimizers' table: srk_adam_slot (`g` the fp32 gradient of this micro-step, `state_off` the tensor's offset in
 * floats into the flat fp32 `acc` buffer -- the layout of the optimizers' flat state; `p`, `step_idx` unused) and srk_adam_block (one
 * workgroup per block).  A window is k micro-steps; `acc` is all zeros at its start.  `op`:
 *     SRK_ACCUM_ADD   (micro-steps 1 .. k-1) : acc = acc + g
 *     SRK_ACCUM_FINAL (micro-step k)         : g = (acc + g) * inv_k;  acc = 0
 * `inv_k` = (float)(1.0 / k), formed in double by the host and passed BY VALUE, 0 < inv_k <= 1 (ADD does not read it).  All fp32, every
 * operation rounded on its own, not contracted: for k a power of two the result is bit for bit what `(loss / k).backward()` k times
 * leaves in `.grad`; for other k it differs by roundings.  FINAL writes the mean IN PLACE of the gradient, where clipping and the
 * optimizers read it, and zeroes `acc` for the next window.  Non-finite values are not special-cased: an inf or NaN of any micro-step
 * reaches the final g (the loss scaler's check behind FINAL then skips the window's update), and `acc` is still zeroed.  Which op runs is
 * the HOST's choice (which hipGraph it replays): nothing on the device counts micro-steps.
 * Traffic: 12 B per parameter (ADD), 16 B (FINAL). */
enum { SRK_ACCUM_ADD = 0, SRK_ACCUM_FINAL = 1 };
typedef struct {
  const srk_adam_slot* slots; const srk_adam_block* blocks; int nslots, nblocks;
  float* acc;
  float inv_k;
  int op;
} srk_grad_accum_args;
int srk_grad_accum(const srk_grad_accum_args* a, srk_stream_t stream);

/* ---- tiled and self-ensemble inference (tiling.py), csrc/tile.hip -------------------------------------------------------------
 * The two data movements around the model's forward when a large image is predicted as a batch of overlapping tiles and / or as the
 * mean over the 8 flips and transposes of the input.  Transform id k: bit 0 reverses W, bit 1 reverses H, bit 2 transposes H and W
 * after the flips.  A tile lives in the TRANSFORMED frame: pixel (Y, X) of transform_k(image) is pixel (y, x) of the image with
 *     (y1, x1) = bit 2 ? (X, Y) : (Y, X);   y = bit 1 ? H-1-y1 : y1;   x = bit 0 ? W-1-x1 : x1.
 * srk_tile_gather: dst[n][c][i][j] = transform_id(src)[c][y0 + i][x0 + j] for the N entries of the DEVICE table, src the LR image
 *   [1][C][H][W], dst the batch [N][C][th][tw]; every tile must lie inside the transformed image.
 * srk_tile_place: src is the batch of SR tiles [N][C][scale*th][scale*tw] (tile n covers rows scale*y0 ..., columns scale*x0 ... of the
 *   transformed HR frame), dst the HR image [1][C][scale*H][scale*W].  Every pixel (y, x) of entry n's owned rectangle
 *   [oy, oy+oh) x [ox, ox+ow) -- given in the UNTRANSFORMED HR image -- receives the tile's value at the matching frame position:
 *   dst = v (accumulate == 0) or dst = dst + weight * v (accumulate != 0: rectangles of one launch must not overlap).  max_oh / max_ow:
 *   the largest oh / ow of the table's entries (host-known; sizes the grid).
 * Both are fp32 NCHW, one launch for any N, 64-bit element offsets (the HR image may pass 2^31 elements). */
typedef struct {
  int y0, x0;                             /* tile origin in the transformed LR frame                        */
  int id;                                 /* transform 0..7                                                 */
  int oy, ox, oh, ow;                     /* place: owned rectangle in the untransformed HR image           */
  int pad_;
} srk_tile_desc;
typedef struct {
  const float* src; float* dst;
  const srk_tile_desc* table;             /* [N] on the device                                              */
  int N, C, H, W;                         /* entries; channels and sides of the (untransformed) LR image    */
  int th, tw;                             /* LR tile sides in the transformed frame                         */
  int scale;                              /* place                                                          */
  int max_oh, max_ow;                     /* place                                                          */
  int accumulate; float weight;           /* place                                                          */
} srk_tile_args;
int srk_tile_gather(const srk_tile_args* a, srk_stream_t stream);
int srk_tile_place(const srk_tile_args* a, srk_stream_t stream);

/* ---- VGG perceptual loss: the glue around srk_conv2d (vgg_loss.py), csrc/vgg_loss.hip ----------------------------------------------
 * Replaces VGGLoss (losses/losses.py:54-117) around its torchvision feature stack: the 3x3 conv + ReLU layers themselves are srk_conv2d
 * launches on frozen packs; these are the passes between them.  All activations are DENSE NHWC in the storage dtype (`dtype`), channels
 * a multiple of 16, so every lane moves 16-byte channel chunks.  No atomics anywhere: every result is bit-identical run to run.
 *   srk_vgg_prepare   : sr and hr ([N][3][H][W] fp32) -> ONE tensor [2N][H][W][16], images 0..N-1 from sr, N..2N-1 from hr;
 *                       channel c < 3 is (x - mean_c) / std_c in fp32 (ImageNet's mean 0.485, 0.456, 0.406 and std 0.229, 0.224,
 *                       0.225), rounded once; channels 3..15 are zero.  Nothing is clamped.  hr NULL: sr alone, [N][H][W][16].
 *   srk_vgg_pool_fwd  : nn.MaxPool2d(2, 2): y[n][i][j][c] = max of x[n][2i..2i+1][2j..2j+1][c], Ho = H / 2, Wo = W / 2 (floor: an odd
 *                       last row / column is dropped).  H, W >= 2.
 *   srk_vgg_pool_bwd  : its backward in GATHER form: gx[n][y][x][c] = gy[n][y/2][x/2][c] when x[n][y][x][c] is the FIRST maximum of its
 *                       window in row-major order (torch's rule) and, with relu_mask, x[n][y][x][c] > 0 (x is a post-ReLU activation:
 *                       the gradient then is the one with respect to the pre-activation); 0 otherwise and in a dropped row / column.
 *   srk_vgg_feat_fwd  : per workgroup, in a fixed slot, the double sum of (fs - fh)^2 (criterion SRK_VGG_L2) or |fs - fh| (SRK_VGG_L1)
 *                       over its share of the n elements of two feature maps; every difference is formed and summed in double.
 *   srk_vgg_feat_finalize : one workgroup: the partials in a fixed order, loss = rescale * sum / n (fp32).
 *   srk_vgg_feat_grad : gf = (fs > 0) ? (fs - fh  |  sign(fs - fh)) : 0 in the storage dtype: the UN-normalised gradient with respect to
 *                       the last pre-activation.  The backward chain is linear, so the factor it lacks is applied at its end:
 *   srk_vgg_image_grad: g [N][H][W][16] (the data gradient of the first conv) -> grad [N][3][H][W] fp32,
 *                       grad = g[c] * (*gout * scale) / std_c with scale = rescale * (2 | 1) / n from the host and gout the upstream
 *                       gradient ON THE DEVICE (a term's weight and the loss scaler's scale arrive through it: capturable).
 * Grids: srk_vgg_blocks(chunks) workgroups of 256 lanes, at most SRK_VGG_BLOCKS_MAX, each walking 16-byte chunks (prepare and
 * image_grad: pixels) with the grid's stride; `partial` has srk_vgg_blocks(n * sizeof(elem) / 16) doubles. */
#define SRK_VGG_BLOCKS_MAX 2048
enum { SRK_VGG_L2 = 0, SRK_VGG_L1 = 1 };
int srk_vgg_blocks(long long chunks);
typedef struct {
  const float* sr; const float* hr;         /* [N][3][H][W] fp32; hr nullable                                 */
  void* dst;                                /* [2N][H][W][16]                                                 */
  int N, H, W;
  int dtype;
} srk_vgg_prepare_args;
int srk_vgg_prepare(const srk_vgg_prepare_args* a, srk_stream_t stream);
/* srk_vgg_relu: x = max(x, 0) in place over n dense elements (n a multiple of 16).  fp32 storage runs a conv of the stack as several
 * srk_conv2d launches over slices of its input channels that add up through `res` (short fp32 chains instead of one of 9 x Cin terms:
 * the accuracy of a blocked sum); the ReLU, which srk_conv2d applies BEFORE `res`, then follows as this pass. */
typedef struct {
  void* x;
  long long n;
  int dtype;
} srk_vgg_relu_args;
int srk_vgg_relu(const srk_vgg_relu_args* a, srk_stream_t stream);
typedef struct {
  const void* x;                            /* [N][H][W][C]: the pool's input                                 */
  void* y;                                  /* fwd out [N][H/2][W/2][C]                                       */
  const void* gy;                           /* bwd in  [N][H/2][W/2][C]                                       */
  void* gx;                                 /* bwd out [N][H][W][C]                                           */
  int N, H, W, C;                           /* C a multiple of 16                                             */
  int relu_mask;                            /* bwd                                                            */
  int dtype;
} srk_vgg_pool_args;
int srk_vgg_pool_fwd(const srk_vgg_pool_args* a, srk_stream_t stream);
int srk_vgg_pool_bwd(const srk_vgg_pool_args* a, srk_stream_t stream);
typedef struct {
  const void* fs; const void* fh;           /* n elements each (n a multiple of 16)                           */
  long long n;
  double* partial;                          /* fwd: written; finalize: read                                   */
  float* loss;                              /* finalize                                                       */
  float rescale;                            /* finalize                                                       */
  int criterion;
  void* gf;                                 /* grad out, n elements                                           */
  int dtype;
} srk_vgg_feat_args;
int srk_vgg_feat_fwd(const srk_vgg_feat_args* a, srk_stream_t stream);
int srk_vgg_feat_finalize(const srk_vgg_feat_args* a, srk_stream_t stream);
int srk_vgg_feat_grad(const srk_vgg_feat_args* a, srk_stream_t stream);
typedef struct {
  const void* g;                            /* [N][H][W][16]                                                  */
  const float* gout;                        /* the upstream gradient, one float on the device                 */
  float* grad;                              /* [N][3][H][W] fp32                                              */
  float scale;
  int N, H, W;
  int dtype;
} srk_vgg_image_grad_args;
int srk_vgg_image_grad(const srk_vgg_image_grad_args* a, srk_stream_t stream);

/* ---- misc ------------------------------------------------------------------------------------------ */
const char* srk_last_error(void);
/* Name of the kernel family the calling thread launched last through srk_conv2d, srk_conv2d_wgrad or srk_unfold_nchw ("" before the
 * first): a thread-local pointer to a string literal, e.g. "conv_ws<2,4,1,1>", "conv_ws<2,4,0,0>x4" (four accumulating passes over a
 * pixel-shuffled input), "conv_igemm<64,3>", "conv_ks", "lk5_fwd", "wgrad_generic<3>".  The names tell apart what the dispatch tells apart;
 * the tests assert on them which side of a dispatch decision ran. */
const char* srk_last_kernel(void);
int srk_version(void);
/* number of compute units of the current device (0 when no device) */
int srk_device_cus(void);

#ifdef __cplusplus
}
#endif
#endif /* SRK_H */
