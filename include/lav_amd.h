/*
 * lav_amd.h - C ABI of liblav_amd.so: the MI355X (gfx950) kernels of the LAV per-frame
 * perception -> prediction -> planning forward path.
 *
 * The reference (dotchen/LAV) has no native code and no FFI: its "operator boundary" for this
 * path is a set of third-party/torch ops called from Python (level B3).
 * Each entry point below replaces one such call site; the reference file:line it replaces is
 * cited on the declaration.  INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add, and lav_amd/_lib.py is that stub as shipped here.
 *
 * Conventions
 *   - plain C: device pointers are raw `void*`/`float*` into HBM, sizes are ints, `stream` is a
 *     hipStream_t passed as void* (NULL = the legacy default stream).  No torch types.
 *   - every call only ENQUEUES work on `stream`; nothing synchronises the host.
 *   - return value: 0 on success, a negative LAV_E* code otherwise; lav_last_error() returns a
 *     thread-local message.  Inputs are never written.
 *   - tensors are dense row-major float32 unless stated; index outputs are int32.
 *   - there is no CPU fallback: on a box without a gfx950 device every entry point fails.
 */
#ifndef LAV_AMD_H
#define LAV_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LAV_ABI_VERSION 50

#define LAV_OK 0
#define LAV_EINVAL (-1)    /* bad argument / unsupported shape */
#define LAV_EHIP (-2)      /* a HIP runtime call failed */
#define LAV_EWORKSPACE (-3)/* workspace too small */

int lav_abi_version(void);
const char *lav_last_error(void);
/* number of HIP devices visible, or a negative error.  Used by the loader to fail loudly. */
int lav_device_count(void);

/* Optional per-kernel timing with HIP events recorded on the launch stream (used by bench.py for
 * the live roofline figure).  lav_profile_enable(slots>0) arms it: the first `slots` launches of each
 * tracked kernel ("pointnet_scatter", "pillar_prep", "conv2d", "paint", "gru_cast", "gru_plan") get an
 * event pair; lav_profile_enable(0) disarms.  lav_profile_read synchronises those events and returns
 * the summed duration and the launch count.  Not part of the reference's surface. */
int lav_profile_enable(int slots);
/* forget recorded launches but keep the (already created) events: call after a warm-up, before the timed region */
int lav_profile_reset(void);
int lav_profile_read(const char *kernel, double *total_ms, int *launches);

/* ------------------------------------------------------------------------------------------
 * 1. PointPillars: dynamic voxelisation + decoration + PointNet + scatter-max + dense canvas.
 *    Replaces PointPillarNet.forward, lav/models/point_pillar.py:92-116, i.e. grid_locations
 *    (:70-79), coords.unique(dim=0) (:82), decorate incl. torch_scatter.scatter_mean (:55-68),
 *    DynamicPointNet incl. torch_scatter.scatter_max (:28-35) and scatter_points (:87-90).
 * ------------------------------------------------------------------------------------------ */
typedef struct lav_grid {
    float min_x, max_x, min_y, max_y; /* metres; keep x in [min_x,max_x), y in [min_y,max_y) */
    float ppm;                        /* pixels per metre */
    int nx, ny;                       /* (max_x-min_x)*ppm, (max_y-min_y)*ppm : number of xi / yi cells */
} lav_grid;

/* PointNet weights with eval-mode BatchNorm1d folded in (host does the folding once):
 *   h1 = relu(f @ w1 + b1),  h2 = relu(h1 @ w2 + b2);  w1 [D+5][C], w2 [C][C], row-major. */
typedef struct lav_pointnet {
    const float *w1, *b1, *w2, *b2;
    int num_input; /* D+5 (16 for the v2 agent) */
    int channels;  /* C (64) */
} lav_pointnet;

/* Bytes of scratch lav_pillar_scatter needs for `batch` clouds of at most `max_points` points.
 *
 * Workspace contract: the head of a pillar workspace holds state that is ZERO AT REST (two sets of arrival counters
 * used alternately and two epoch words), which is what lets a call run as two launches with no memset.  Zero-fill a
 * workspace ONCE after allocating it (lav_pillar_workspace_init, or any memset), keep it for ONE (batch, grid) geometry
 * (max_points may vary up to the size it was allocated for) and do not write to it between calls; every call leaves it
 * clean for the next one.  Re-run lav_pillar_workspace_init to reuse the memory for another geometry or after a
 * failed launch.  Calls sharing a workspace must be ordered on one stream. */
size_t lav_pillar_workspace_bytes(int batch, int max_points, const lav_grid *grid);
int lav_pillar_workspace_init(void *workspace, size_t workspace_bytes, void *stream);

/*
 * points      [batch][max_points][D]   (a single cloud: batch=1, max_points=N)
 * h_num_points host array [batch]: only the first h_num_points[b] rows of cloud b are used (:98)
 * canvas      out [batch][C][ny][nx]; every element is written (empty cells = 0)
 * Optional index outputs (NULL to skip; they cost extra passes and exist for parity/training):
 *   unique_coords out [<= total kept][3] rows (b, xi, yi) sorted lexicographically  (:82)
 *   inverse       out [total kept]  pillar row of each kept point, in input order   (:82)
 *   counts        out [2] = { number of pillars P, number of kept points }
 */
int lav_pillar_scatter(const float *points, const int *h_num_points, int batch, int max_points, int D,
                       const lav_grid *grid, const lav_pointnet *net, float *canvas,
                       int *unique_coords, int *inverse, int *counts,
                       void *workspace, size_t workspace_bytes, void *stream);
/* The same call leaving a BOUND of the canvas for the layer that reads it (round 6): amax_parts[0 .. lav_pillar_amax_count(batch, grid))
 * receives, per workgroup of the canvas kernel, the largest finite value its PointNet produced (>= every value it wrote; the
 * canvas holds ReLU outputs, so this bounds |canvas|).  LAV_CONV_F16X3 layers take their activation scale from such parts
 * (lav_conv2d_amax) instead of measuring their input with a launch of their own: ConvBackbone's first convolution,
 * team_code_v2/models/lidar.py:57.  amax_parts NULL = lav_pillar_scatter. */
int lav_pillar_amax_count(int batch, const lav_grid *grid);
int lav_pillar_scatter_amax(const float *points, const int *h_num_points, int batch, int max_points, int D,
                            const lav_grid *grid, const lav_pointnet *net, float *canvas,
                            int *unique_coords, int *inverse, int *counts, float *amax_parts,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * 2. Point painting: LiDAR->camera projection + semantic gather for up to 4 cameras.
 *    Replaces InferModel.forward_paint / point_painting / CoordConverter.forward,
 *    team_code_v2/model_inference.py:44-50, 75-93, 280-297.
 * ------------------------------------------------------------------------------------------ */
typedef struct lav_camera {
    float K[9];    /* row-major 3x3 intrinsics                       (model_inference.py:259-262) */
    float l2w[16]; /* row-major 4x4 lidar_to_world                    (:264-266) */
    float w2c[16]; /* row-major 4x4 world_to_cam                      (:268-271) */
} lav_camera;

/*
 * lidar    [n][lidar_dim]  (xyz in columns 0..2; lidar_dim >= 3)
 * sem      [ncam][sem_c+1][h][w] softmax probabilities; channel 0 is the "other" class
 * fused    out [n][lidar_dim + sem_c] = cat(lidar, painted) where, per camera in order (later
 *          cameras overwrite), painted = sem[cam][1+c][v][u] * (1 - sem[cam][0][v][u]) for points
 *          whose truncated (u, v, depth) satisfy depth>=0, 0<=u<w, 0<=v<h; else 0.
 * uvz      optional out [ncam][n][3] int32 truncated projections (INT32_MIN where the reference's
 *          .long() is out of range); NULL to skip.
 */
int lav_paint(const float *lidar, int n, int lidar_dim, const float *sem, int ncam, int sem_c, int h, int w,
              const lav_camera *h_cams, float *fused, int *uvz, void *stream);

/* ------------------------------------------------------------------------------------------
 * 3. GRU waypoint decoders.  Replaces UniPlanner.cast (team_code_v2/models/uniplanner.py:288-308),
 *    UniPlanner.plan/_plan (:255-286) and the cuDNN GRU calls inside them.
 *    PyTorch GRU parameter layout: w_ih [3H][I], w_hh [3H][H], b_ih [3H], b_hh [3H], gates r,z,n.
 * ------------------------------------------------------------------------------------------ */
/*
 * cast: for each of num_cmds GRUs (I=embd_dim, H=hidden): constant input embd[b] at every step,
 *       h0 = 0, T steps; locs = cumsum_t( mlp_w @ h_t + mlp_b ).
 * embd [B][embd_dim]; w_ih [num_cmds][3H][embd_dim]; w_hh [num_cmds][3H][H]; b_ih,b_hh [num_cmds][3H];
 * mlp_w [num_cmds][2][H]; mlp_b [num_cmds][2];  out [B][num_cmds][T][2]
 */
int lav_gru_cast(const float *embd, int B, int embd_dim, int H, int num_cmds, int T,
                 const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                 const float *mlp_w, const float *mlp_b, float *out,
                 void *workspace, size_t workspace_bytes, void *stream);
size_t lav_gru_cast_workspace_bytes(int B, int embd_dim, int H, int num_cmds, int T);
/*
 * embed + cast: the tail of the embedder and everything that hangs on it, in one launch per batch
 * (uniplanner.py:36-40 AdaptiveAvgPool2d + Flatten, :50-53 cast_cmd_pred, :288-308 cast;
 * model_inference.py:164-165, 240-251 transform_points + translate).
 * feat [B][embd_dim][hw]: the embedder's last feature map (hw pixels per channel; hw = 1: the embedding itself);
 * embd_out [B][embd_dim] or NULL: its spatial mean; cmd_w [num_cmds][embd_dim], cmd_b [num_cmds], cmds_out [B][num_cmds]
 * (all three or none): sigmoid(cmd_w . embd + cmd_b); oris [B], locs [B][2] (each optional): every decoded waypoint
 * (x, y) becomes (x cos o - y sin o, x sin o + y cos o) + loc.  Everything else as lav_gru_cast; honours lav_batch_limit.
 */
int lav_embed_cast(const float *feat, int B, int embd_dim, int hw, float *embd_out, int H, int num_cmds, int T,
                   const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                   const float *mlp_w, const float *mlp_b, const float *cmd_w, const float *cmd_b, float *cmds_out,
                   const float *oris, const float *locs, float *out, void *stream);

/*
 * plan: GRU(I=4 -> H), h0 = embd[b]; iteration it, command c:
 *         u_t = [ nxp[b]*ppm/crop_size*2-1 , loc_{it-1}[b][c][t] ],  loc_{-1} = cast_locs
 *         loc_it[b][c] = cumsum_t(mlp(h_t)) + loc_{it-1}[b][c]
 * cmd >= 0: only that command branch is evaluated (branches never interact) and `out` is
 *           [B][iters][1][T][2];  cmd = -1: all branches, out [B][iters][num_cmds][T][2].
 * embd [B][H]; nxp [B][2]; cast_locs [B][num_cmds][T][2]; w_ih [3H][4]; w_hh [3H][H]; mlp_w [2][H].
 */
int lav_gru_plan(const float *embd, const float *nxp, const float *cast_locs, int B, int H, int num_cmds, int T,
                 int iters, int cmd, float pixels_per_meter, float crop_size,
                 const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                 const float *mlp_w, const float *mlp_b, float *out,
                 void *workspace, size_t workspace_bytes, void *stream);
size_t lav_gru_plan_workspace_bytes(int B, int H, int num_cmds, int T);
/* A plan workspace must be ZERO before its first use and belongs to one stream.  Its first 512 bytes are a control block:
 * [0, 256) sticky counters {aborted persistent launches, persistent launches} since it was zero-filled, [256, 512) the status
 * and diagnosis words of the last persistent launch (cleared at every launch).  Behind it, with R = B * (1 or num_cmds) state rows:
 * the persistent launch keeps two buffers of R*H 8-byte granules; the step-per-launch path the state sequence [T][R][H] floats - with
 * 512 + T*R*H*4 bytes it runs - and, from 16 rows on, the MFMA step's initial state [R][H] and inputs [R][T][4] (without room for
 * them the rows run on the slower VALU step kernel).  lav_gru_plan_workspace_bytes covers every path: 512 + the largest of these,
 * rounded up to 256. */
/*
 * lav_gru_plan runs all iters*T dependent steps in ONE persistent launch when B*(1 or num_cmds) <= 6: its H/8 workgroups
 * exchange the hidden state through HBM and must be co-resident.  Every wait is bounded; a launch that times out (the chip
 * oversubscribed by other streams) fills the WHOLE `out` with NaN and raises the status word of its workspace:
 *   lav_gru_plan_status  copies that word to *h_status (0 = completed, 1 = aborted) - it SYNCHRONISES `stream`;
 *   lav_gru_plan_steps   same contract as lav_gru_plan on the step-per-launch path (no co-residency requirement, ~10 % slower):
 *                        what a caller runs after an abort.
 */
int lav_gru_plan_status(const void *workspace, size_t workspace_bytes, int B, int H, int num_cmds, int cmd,
                        int *h_status, void *stream);
/* lav_gru_plan_diag: the 16 diagnosis words of the last persistent launch (SYNCHRONISES `stream`): [0] status, [1] workgroups
 * that entered the kernel, [2] 1 + workgroup / [3] wave / [4] step epoch of the first wave that gave up, [5] its spin count,
 * [6] the state granule it was waiting for, [7] the tag it last saw there, [8] microseconds from its kernel entry to the abort,
 * [9] workgroups that ran to completion (H/8 after a good launch); sticky since the workspace was zero-filled: [10] aborted
 * launches, [11] all persistent launches (a plan workspace must be ZERO before its first use).  No counterpart in the reference (cuDNN's GRU cannot
 * time out); it exists so that an abort can be told apart from lost co-residency vs a lost hand-off. */
int lav_gru_plan_diag(const void *workspace, size_t workspace_bytes, int B, int H, int num_cmds, int cmd,
                      int *h_words16, void *stream);
int lav_gru_plan_steps(const float *embd, const float *nxp, const float *cast_locs, int B, int H, int num_cmds, int T,
                       int iters, int cmd, float pixels_per_meter, float crop_size,
                       const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                       const float *mlp_w, const float *mlp_b, float *out,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * 3b. GRU over a sequence with a saved tape - the TRAINING side of the same decoders: what nn.GRU (cuDNN there, MIOpen
 *     here) does under UniPlanner.cast / _plan / BEVPlanner in train mode (team_code_v2/models/uniplanner.py:255-308,
 *     lav/models/bev_planner_v2.py, called from lav/lav_final_v2.py:140-259 and lav/lav_privileged_v2.py:110-159).
 *     One launch per time step (recurrent GEMM on MFMA fused with the gates); the input projection and the weight
 *     gradients are plain GEMMs over all (row, step) pairs and are the caller's (see lav_amd/ops.py:gru_seq).
 *
 *     x      : input-side pre-activations W_ih u + b_ih, gate order (r, z, n): [R][T][3H] when x_per_step, else [R][3H]
 *              (the same input at every step - the cast decoders)
 *     h0     : [R][H];  w_hh [3H][H], b_hh [3H];  out [R][T][H];  tape [R][T][4][H] = (r, z, n, W_hn h + b_hn) per step
 *              (may be NULL for an inference-only forward)
 *   backward : dout [R][T][H] -> dx [R][T][3H] (gradient of x per step; sum over T for a shared x), dgh [R][T][3H]
 *              (gradient of the recurrent-side pre-activations: dW_hh = dgh^T [h0, out[:, :-1]], db_hh = sum dgh), dh0 [R][H].
 *              w_hh_t = W_hh transposed, [H][3H].  H must be a multiple of 16.  No atomics: results are bit-reproducible.
 */
int lav_gru_seq_forward(const float *x, int x_per_step, const float *h0, const float *w_hh, const float *b_hh,
                        int R, int T, int H, float *out, float *tape, void *stream);
size_t lav_gru_seq_backward_workspace_bytes(int R, int H);
int lav_gru_seq_backward(const float *dout, const float *tape, const float *out, const float *h0, const float *w_hh_t,
                         int R, int T, int H, float *dx, float *dgh, float *dh0,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * 4. 2-D convolutions on the matrix cores.  fp32 in, fp32 out, fp32 accumulation; the products are either exact fp32
 *    (v_mfma_f32_32x32x2_f32; precision = LAV_CONV_F32) or - the default, LAV_CONV_BF16X6 - each operand is split exactly into
 *    three bf16 pieces and the six leading partial products run on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16): the same
 *    accuracy class as the fp32 chain (max error 3e-7 vs 6e-7 of sum |a||b| at K = 1152) at up to twice its rate; the launch
 *    plan picks per layer and shape among the tiled, direct and split-operand kernels.  Replaces the cuDNN calls behind ConvBackbone / Head
 *    (team_code_v2/models/lidar.py:48-161) and, with the same kernel, the ResNet-18 embedder
 *    (lav/models/resnet.py:39-82,235-247).  NCHW activations.
 *
 *    y = epilogue( conv(x, w) ),  epilogue in this order (each optional):
 *        + bias[co] -> ReLU (relu_pre) -> * scale[co] + shift[co] -> + residual -> ReLU (relu_post)
 *        -> sigmoid
 *    (the reference's BEV blocks are Conv -> ReLU -> BatchNorm, lidar.py:57-60, i.e. relu_pre +
 *    scale/shift; its ResNet blocks are Conv -> BatchNorm (-> +identity) -> ReLU, i.e. scale/shift
 *    (+residual) + relu_post.)
 * ------------------------------------------------------------------------------------------ */
typedef struct lav_conv {
    int batch;
    int in_c_total, in_c_offset, cin; /* x is [batch][in_c_total][h][w]; channels [in_c_offset, +cin) are read */
    int h, w;
    int cout, kh, kw;
    int stride, pad_h, pad_w, dil_h, dil_w;
    int transposed, out_pad;             /* 1: ConvTranspose2d(stride, padding=pad_h/pad_w, output_padding) */
    int out_c_total, out_c_offset;       /* y is [batch][out_c_total][oh][ow]; channels [out_c_offset, +cout)
                                            are written (fused torch.cat, lidar.py:143) */
    int relu_pre, relu_post;
    int sigmoid;       /* 0: none; k > 0: sigmoid on output channels >= k-1 of this convolution (1 = all of them) */
    int target_cus;    /* 0 = plan for the whole chip (256 CUs); n: plan tiles / split-K to fill n CUs - for layers of a
                          network that runs on a side stream next to another network's kernels */
    float pad_value;   /* what out-of-image taps read (0 = zero padding).  A network whose input normalisation x' = s*x + t
                          has been folded into its first convolution pads the RAW image with -t/s instead */
    int precision;     /* how the fp32 contraction is evaluated: LAV_CONV_F32 = v_mfma_f32_32x32x2_f32 only (bit-for-bit an
                          fmaf chain); LAV_CONV_BF16X6 = layers whose plan favours it run on the bf16 matrix cores with every
                          fp32 operand split exactly into three bf16 pieces and the six leading partial products accumulated
                          in fp32 (error of an fp32 dot product, 2.4x the matrix rate; fp32 subnormal inputs are flushed; every
                          finite input up to FLT_MAX is split exactly; an Inf or NaN activation / weight gives NaN in the
                          outputs it reaches, where LAV_CONV_F32 and the reference's cuDNN path propagate Inf as Inf - through
                          the epilogue too: relu_pre / relu_post keep a NaN as torch.relu does (csrc/common.hpp relu_nan), in
                          every kernel of the library with a ReLU or a 2x2 max-pool, the train-mode BatchNorm included;
                          tests/test_gpu_nonfinite.py.  Not so where NaN has a meaning of its own: the pillar kernels (NaN =
                          absent point) and lav_extract_peaks (a NaN is ignored inside every window), nor in backward kernels);
                          0 = the library default (environment LAV_CONV_PRECISION = f32 | bf16x6, default bf16x6).  The
                          packed weights of a layer depend on it: pack and run with the same descriptor.  Launch note: a
                          workgroup of the split-operand kernel asks for the LDS its tiles need and no more, so kernels of
                          other streams that use LDS may run beside it on a CU (the wrong results once measured in such
                          neighbours on gfx950 came from packed fp32 instructions, which the library no longer contains:
                          DESIGN 4.4c) */
} lav_conv;
#define LAV_CONV_F32 1
#define LAV_CONV_BF16X6 2
#define LAV_CONV_F16X3 3   /* as BF16X6, and wherever the plan is the split kernel (round 5: the head convolution's plan only; round 6:
                              every split plan - any stride, tile, split-K, tap pairs, the classes of a transposed convolution) each
                              operand is TWO fp16 pieces scaled by a power of two taken from the tensor's largest finite magnitude,
                              three products: half the matrix instructions at 22 bits per operand.  Precision (tests/
                              test_gpu_f16x3_contract.py): the scale s puts the tensor's largest magnitude into [2^14, 2^15) (exponent
                              floored: s >= 2^-115), and an element keeps an ABSOLUTE error of up to 2^-25 s (fp16's subnormal
                              quantum), i.e. 2^-40 .. 2^-39 of the tensor's maximum, so the bound is two-term:
                                |y - y_exact| <= 2e-6 sum|w||x| + 2^-25 (s_x sum|w| + s_w sum|x|)   (sums over the receptive field)
                              (measured: at most 0.21 of the second term where it dominates).  Outputs whose inputs and weights lie
                              within 2^-20 of their tensors' maxima keep the 2e-6 of sum|w||x| bar of BF16X6 (measured <= 2.6e-7);
                              at 2^-30 the error reached 2.8e-4 of sum|w||x|.  fp32 SUBNORMAL activations are not flushed (unlike
                              BF16X6): they are scaled like any value and count when the scaled value is above 2^-25, i.e. when the
                              tensor's maximum is small; Inf / NaN make the outputs they reach non-finite - the epilogue's ReLUs keep them -
                              and change no other bit (the scale hand-offs take the largest FINITE magnitude).
                              Magnitudes up to FLT_MAX are exact as in BF16X6: the epilogue applies s_x s_w as two balanced powers
                              of two, so neither it nor acc * s_x overflows where y does not.  The activations' magnitude comes from the launches that
                              wrote them (lav_conv2d_amax below) or, without that, from one measuring launch in front of the
                              convolution.  Re-packing on the device: lav_conv_repack_scratch (the weights' magnitude is measured first) */

/* output spatial size of the convolution */
int lav_conv_out_hw(const lav_conv *c, int *oh, int *ow);
/* number of floats of the packed weight buffer */
size_t lav_conv_packed_weight_floats(const lav_conv *c);
/* host-side repack of a PyTorch-layout weight (Conv2d: [cout][cin][kh][kw]; ConvTranspose2d:
 * [cin][cout][kh][kw]) into the kernel's layout [class][cout block of 32][tap][8-channel group][lane][channel pair] -
 * the order in which the MFMA A operands are consumed, so both kernels fetch 16 bytes per lane.  Pure host code. */
int lav_conv_pack_weights(const lav_conv *c, const float *h_weight, float *h_packed);
/* Re-packing on the device, for callers whose weights change in HBM (a training run that evaluates its student through these
 * kernels after every optimiser step, lav/lav_final_v2.py:228-236): lav_conv_pack_map (host, once per layer) fills
 * lav_conv_pack_map_ints(c) ints - for every slot of the packed buffer the index of the PyTorch-layout weight it holds, -1 for
 * padding; lav_conv_repack gathers (and, for LAV_CONV_BF16X6, splits) the packed buffer from the device-resident weight with
 * that map in one launch: bit-identical to lav_conv_pack_weights + upload.  lav_bn_fold: the eval-mode BatchNorm affine
 * scale = gamma / sqrt(var + eps), shift = beta - mean * scale (float64 arithmetic) of n channels, on the device. */
size_t lav_conv_pack_map_ints(const lav_conv *c);
int lav_conv_pack_map(const lav_conv *c, int *h_map);
int lav_conv_repack(const lav_conv *c, const float *d_weight, const int *d_map, float *d_packed, void *stream);
/* the same with 512 floats of device scratch (round 6): what a LAV_CONV_F16X3 layer needs - its fp16 section is scaled by the weights'
 * largest magnitude, which is measured on the device first (lav_conv_repack refuses such a layer) */
int lav_conv_repack_scratch(const lav_conv *c, const float *d_weight, const int *d_map, float *d_packed, float *d_parts, size_t parts_floats,
                            void *stream);
int lav_bn_fold(const float *mean, const float *var, const float *gamma, const float *beta, double eps, int n, float *scale,
                float *shift, void *stream);
/* introspection of the launch plan (host only, no device access): info[0..8] = { MP, MC, row-blocked tiles,
 * staged tile width, staged tile rows, LDS bytes, split-K factor, taps per weight slab, chunks per stage }; small layers
 * that take the direct kernel (whole batch in one GEMM dimension, operands straight from L2, no LDS staging) report
 * info[0] = 0 and info[1] = waves per workgroup.  Fails exactly when lav_conv2d would reject the shape. */
int lav_conv_tile_info(const lav_conv *c, int *info);
/* scratch for the split-K partial sums of small-output / deep-channel layers (0 when the layer is not split) */
size_t lav_conv_workspace_bytes(const lav_conv *c);
/* x, y, w_packed: device.  bias / scale / shift: [cout] device or NULL.  residual: same shape and
 * channel window as y, or NULL. */
int lav_conv2d(const lav_conv *c, const float *x, const float *w_packed, const float *bias, const float *scale,
               const float *shift, const float *residual, float *y, void *workspace, size_t workspace_bytes,
               void *stream);
/* lav_conv2d with the scale hand-off of LAV_CONV_F16X3 (round 6; replaces nothing in the reference - its cuDNN layers compute in
 * fp32 - it is what lets a CHAIN of layers, team_code_v2/models/lidar.py:110-143, lav/models/resnet.py:41-85, run on fp16 pieces
 * without a pass over the activations per layer).  amax_out (device, lav_conv_amax_count(c) floats, or NULL): the launch leaves
 * the largest finite |y| of each of its workgroups there (from its epilogue; from the split-K reduce pass; for the few plans with
 * neither, measured by one more launch) - rows beyond lav_batch_limit contribute 0, nothing needs zeroing.  amax_in / amax_in_count
 * (device, or NULL / 0): such maxima of the tensor(s) x was assembled from - any values whose maximum bounds max |x| (e.g. the
 * maxima of a tensor that x is a max-pooling, a crop or a bilinear resampling of); a LAV_CONV_F16X3 layer on the split kernel takes
 * its power-of-two scale from them instead of measuring x (other layers ignore them).  A bound that is too small would overflow
 * fp16 (a wrong, possibly finite y: the pieces saturate); one that is 2^k too large costs k of the 22 operand bits.  The library's
 * Python engines keep a bound only while it holds: a tensor carries its producer's bound with the tensor's version and the buffer's
 * generation (lav_amd/ops.py tag_amax / amax_of), and concurrent streams never share a buffer. */
#define LAV_AMAX_PARTS 512   /* floats lav_absmax_parts writes */
int lav_absmax_parts(const float *x, long n, float *parts, void *stream);   /* maxima of the finite |x[0 .. n)| in LAV_AMAX_PARTS parts: one launch */
int lav_conv_amax_count(const lav_conv *c);
int lav_conv2d_amax(const lav_conv *c, const float *x, const float *w_packed, const float *bias, const float *scale,
                    const float *shift, const float *residual, float *y, void *workspace, size_t workspace_bytes,
                    const float *amax_in, int amax_in_count, float *amax_out, void *stream);

/* Grouped ConvTranspose2d with few output channels (memory bound, vector-ALU kernel): group g maps input channels
 * [g*cin/groups, (g+1)*cin/groups) to cout_per_group[g] (1..8) output channels; y is [batch][sum cout][oh][ow] with the
 * groups' channels in order.  weight: the groups' PyTorch-layout ConvTranspose2d weights [cin/groups][cout_g][k][k]
 * concatenated (device).  bias: [sum cout] device or NULL.  sigmoid_from: output channels >= it get a sigmoid, -1 = none,
 * -2 = softmax over each group's channels (the class probabilities the agent takes from ERFNet, lav_agent_fast.py:264).
 * (kernel, stride) = (3, 2) or (2, 2).  cout_per_group is a host array.  Replaces the four head tails
 * ConvTranspose2d(64, out, 3, 2, 1, 1) of team_code_v2/models/lidar.py:30-33 (one launch for all heads) and ERFNet's
 * output layer lav/models/erfnet.py:137. */
int lav_deconv_grouped(int batch, int cin, int h, int w, int groups, const int *cout_per_group, int kernel, int stride,
                       int pad, int out_pad, const float *x, const float *weight, const float *bias, int sigmoid_from,
                       float *y, void *stream);

/* ------------------------------------------------------------------------------------------
 * 5. Rotated crop of the BEV feature map around each actor.  Replaces crop_feature
 *    (team_code_v2/model_inference.py:204-238; same maths team_code_v2/models/uniplanner.py:310-352):
 *    theta = k*R(ori) about the (offset_x, offset_y) pivot, k = crop/H, affine_grid + bilinear grid_sample,
 *    zeros outside, align_corners=True.
 *    feat [feat_batch][C][H][W] (feat_batch = 1: the one map is shared by all n crops, the reference's
 *    features.expand(N, ...)); locs [n][2] metres, oris [n] radians (device); out [n][C][crop][crop].
 * ------------------------------------------------------------------------------------------ */
int lav_crop_rotate(const float *feat, int feat_batch, int C, int H, int W, const float *locs, const float *oris, int n,
                    float pixels_per_meter, int crop, float offset_x, float offset_y, float *out, void *stream);
/* Training form (lav/models/uniplanner.py:84-95, bev_planner_v2.py:91-104): crop n is taken from map map_index[n]
 * (int32, device) of feat [num_maps][C][H][W] - the reference materialises features.expand(N, ...)[mask], one 39 MB
 * copy of the feature map per sampled vehicle, before cropping.  The backward spreads grad_out [n][C][crop][crop] over
 * the source pixels of grad_feat [num_maps][C][H][W] (zeroed by the call; fp32 atomics, like torch's grid_sampler). */
int lav_crop_rotate_indexed(const float *feat, int num_maps, const int *map_index, int C, int H, int W, const float *locs,
                            const float *oris, int n, float pixels_per_meter, int crop, float offset_x, float offset_y,
                            float *out, void *stream);
int lav_crop_rotate_backward(const float *grad_out, int num_maps, const int *map_index, int C, int H, int W, const float *locs,
                             const float *oris, int n, float pixels_per_meter, int crop, float offset_x, float offset_y,
                             float *grad_feat, void *stream);

/* ------------------------------------------------------------------------------------------
 * 6. Per-frame glue of LAVAgent.run_step between the big kernels (one launch each).
 *
 * lav_merge_ticks: cur = cat([tick, prev]) with the ego-vehicle box removed, then prev = tick
 *    (team_code_v2/lav_agent_fast.py:240-247 and preprocess() :450-452).  Removed points are marked x = NaN
 *    instead of being compacted: they fail every range test downstream exactly like absent points, and the
 *    row count stays static.  tick, prev [rows][4], cur [2*rows][4] (device).
 *
 * lav_stack_sweeps: get_stacked_lidar() (lav_agent_fast.py:363-383) with move_lidar_points() (:547-565).
 *    fused [rows][8] is the newly painted sweep; ring [slots][rows][8] the history; d_slot (1 int64, device):
 *    ring slot the new sweep is stored to; d_sweeps [num_sweeps] int64 (device): ring slots of sweeps t, t-5, t-10
 *    (d_sweeps[0] is ignored: sweep 0 is `fused`); d_R [num_sweeps][3][3], d_t [num_sweeps][3] (device): xyz' = xyz@R + t.
 *    out [num_sweeps*rows][8 + num_sweeps] = (xyz', features, one-hot sweep index).
 *
 * lav_extract_peaks: extract_peak() (team_code_v2/model_inference.py:189-202: 7x7 max-pool NMS, top-15 by
 *    score) over `ncls` heat-map planes [ncls][h][w] (apply_sigmoid: logits in, scores out) plus the gathers of
 *    det_inference() (:95-121) from size [size_c][h][w] and ori [ori_c][h][w].
 *    out [ncls][max_det][3 + size_c + ori_c] = (score, x, y, size..., ori...), rows by descending score, ties by
 *    ascending pixel index; if a plane has fewer than max_det non-suppressed pixels the remaining rows carry
 *    score -1e5 and zeros.  A NaN is ignored inside every window, and a NaN pixel itself survives and sorts by its bit
 *    pattern (a +NaN before every number).  The last 256 bytes of the workspace are counters: zero before the first use, left zero.
 * ------------------------------------------------------------------------------------------ */
int lav_merge_ticks(const float *tick, float *prev, int rows, int dim, float *cur, void *stream);
int lav_stack_sweeps(const float *fused, float *ring, const long *d_slot, const long *d_sweeps, const float *d_R,
                     const float *d_t, int num_sweeps, int rows, int dim, float *out, void *stream);
size_t lav_extract_peaks_workspace_bytes(int ncls, int h, int w);
int lav_extract_peaks(const float *heat, int ncls, int h, int w, int ks, int max_det, int apply_sigmoid,
                      const float *size, int size_c, const float *ori, int ori_c, float *out, void *workspace,
                      size_t workspace_bytes, void *stream);

/* lav_heads_at_peaks (ABI 44): heads of the form conv3x3(cin -> hidden, padding 1, no bias) -> ReLU -> y * scale + shift (the folded
 *    eval BatchNorm, fmaf(max(v, 0), scale, shift)) -> ConvTranspose2d(hidden -> outs, kernel 3, stride 2, padding 1, output_padding 1)
 *    evaluated ONLY at the pixels named by peak rows, instead of on the whole [2h][2w] map: an output pixel depends on 1, 2 or 4 hidden
 *    pixels by the parity of its coordinates, each hidden pixel on a 3 x 3 x cin window of the zero-padded feature map.
 *    feat [cin][h][w] float32; rows [ncls][max_det][3] = (score, x, y) as lav_extract_peaks writes them with size_c = ori_c = 0;
 *    per head g < nheads (1 .. 4): w1_packed[g] the first convolution's weights as [kpad][64] floats, kpad = 9 cin rounded up to 128,
 *    row k = ci * 9 + ky * 3 + kx, column = hidden channel, zeros elsewhere (lav_heads_at_peaks_packed_floats(cin, hidden) floats; 0 for
 *    bad sizes); scale[g], shift[g] [hidden[g]]; wt[g] the transposed convolution's weights [hidden[g]][outs[g]][3][3]; bias[g]
 *    [outs[g]] or NULL; hidden[g] in 1 .. 64, outs[g] in 1 .. 4 (host arrays of device pointers / ints, read before the call returns).
 *    out [ncls][max_det][3 + sum of outs]: columns 0 .. 2 copied, then head 0's values, head 1's, ... - the rows lav_det_decode takes.
 *    A row with score <= -1e4 (lav_extract_peaks' "no candidate" rows carry -1e5) or with x / y non-finite or outside [0, 2w) x [0, 2h)
 *    gets zeros behind its three columns; no address is formed from an unchecked row value.  Plain fp32 fmaf chains, combined in an order fixed
 *    by (cin, hidden): results do not depend on the other rows and two launches are bit-identical.  No workspace. */
size_t lav_heads_at_peaks_packed_floats(int cin, int hidden);
int lav_heads_at_peaks(const float *feat, int cin, int h, int w, const float *rows, int ncls, int max_det, int nheads,
                       const float *const *w1_packed, const float *const *scale, const float *const *shift, const float *const *wt,
                       const float *const *bias, const int *hidden, const int *outs, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * 6b. Single-query attention pooling of the brake net.  Replaces Attention.forward, lav/models/attention.py:21-38
 *     (called twice per frame from RGBBrakePredictionModel.forward, team_code_v2/models/rgb.py:69-70): Linear(C -> 2C) key/value
 *     projection, positional encoding on the keys, one learned query per head, soft-max over the h*w tokens, weighted sum.
 *     With one fixed query per head the key projection folds into the query and the value projection moves behind the
 *     weighted sum (exact algebra, prepared once from the weights on the host):
 *       u         [heads][C]  = scale * W_k,h^T q_h
 *       dots_bias [heads][N]  = scale * q_h . (b_k,h + PE[n])
 *       out[b][h*dh + d]      = W_v[h*dh + d] . (sum_n softmax_n(u_h . x[b][:, n] + dots_bias[h][n]) x[b][:, n]) + b_v[h*dh + d]
 *     x [batch][C][N] (an NCHW map, N = h*w tokens), w_v [C][C] (rows = outputs, PyTorch Linear layout), out [batch][C].
 * ------------------------------------------------------------------------------------------ */
int lav_attn_pool(const float *x, int batch, int C, int N, int heads, const float *u, const float *dots_bias,
                  const float *w_v, const float *b_v, float *out, void *stream);

/* Train mode of the same pooling (ABI 30; the brake-net trainer, lav_amd.train.hipnn.attn_pool_train).  q [heads][dh] (dh = C / heads,
 * even), w_kv [2C][C] and b_kv [2C] = linear_kv (keys first), pe [N][dh] the positional encoding, scale = dh^-1/2: the LIVE
 * parameters, folded on the device (no host preparation).  C <= 1024 (any multiple of the heads), N <= 4096.  fp32 arithmetic, every
 * sum in an order fixed by the shape, no atomics: bit-reproducible.
 *   forward:  u [heads][C], dots_bias [heads][N] (the folding, kept for the backward), out [batch][C], and the saved
 *             p [batch][heads][N] (soft-max over the tokens) and xbar [batch][heads][C] (= sum_n p x_n).  Two launches.
 *   backward: from dout [batch][C]: dx [batch][C][N], dq [heads * dh], dw_kv [2C][C], db_kv [2C] (the parameter gradients summed
 *             over the batch, images in order).  Four launches; workspace lav_attn_train_workspace_bytes. */
size_t lav_attn_train_workspace_bytes(int batch, int C, int N, int heads);
int lav_attn_train_forward(const float *x, int batch, int C, int N, int heads, const float *q, const float *w_kv, const float *b_kv,
                           const float *pe, float scale, float *u, float *dots_bias, float *out, float *p, float *xbar, void *stream);
int lav_attn_train_backward(const float *x, int batch, int C, int N, int heads, const float *q, const float *w_kv, const float *b_kv,
                            const float *pe, float scale, const float *u, const float *p, const float *xbar, const float *dout, float *dx,
                            float *dq, float *dw_kv, float *db_kv, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Health counter of a frame: counter2[0] += how many of the n (<= 8) float tensors hold a NaN or an Inf, counter2[1] += 1.
 * Sticky and device resident: enqueued behind a frame's last kernels (it is part of the HIP graphs), read by the host when it
 * likes.  The reference checks its waypoints on the host every tick (lav_agent_fast.py:325-328, np.isnan after .cpu()); this is
 * the same question asked without a device->host copy per tensor, so that a benchmark loop can prove every timed frame finite.
 * A tensor of zero elements is finite, and its pointer may be NULL.
 */
int lav_nonfinite_count(int n, const float *const *tensors, const long *numel, int *counter2, void *stream);

/* Frame glue that replaces library launches inside the frame graphs:
 * lav_maxpool3x3s2: nn.MaxPool2d(3, 2, 1) of the ResNet stems (lav/models/resnet.py:161,236), x [batch][channels][h][w] ->
 *     y [batch][channels][(h-1)/2+1][(w-1)/2+1]; honours lav_batch_limit.
 * lav_channel_affine: y = x * scale[c] + shift[c] on [batch][channels][plane] (plane % 4 == 0): the brake net's
 *     `normalize(rgb / 255)` (team_code_v2/models/rgb.py:71-72) in one pass.
 * lav_copy_many: up to 8 device-to-device copies (16-byte aligned pointers, sizes multiples of 4) in ONE launch: a tick's sensor tensors
 *     into the static buffers the frame graphs read (lav_agent_fast.py:233-277 hands them over as fresh tensors). */
int lav_maxpool3x3s2(const float *x, int batch, int channels, int h, int w, float *y, void *stream);
int lav_channel_affine(const float *x, int batch, int channels, long plane, const float *scale, const float *shift, float *y, void *stream);
int lav_copy_many(int n, const void *const *src, void *const *dst, const size_t *bytes, void *stream);
/* lav_stage_many: up to 8 strided tensors of at most 4 dimensions (float32, or uint8 converted to float32) -> contiguous float32
 *     buffers in ONE launch.  dims[4 n] (outermost first, leading 1s), strides[4 n] in source elements.  The camera tensors
 *     of a tick are channels-last views (lav_agent_fast.py:252-277: stack / permute / float). */
int lav_stage_many(int n, const void *const *src, float *const *dst, const int *dims, const long *strides, const int *src_is_u8,
                   void *stream);
/* lav_stage_many_block (ABI 28): the same launch, with up to 256 bytes of HOST data (a multiple of 4) riding in its kernel arguments and
 *     written to block_dst in HBM by the kernel: the per-tick sweep indices and float32 poses that get_stacked_lidar computes on the host
 *     (lav_agent_fast.py:363-383) - an upload of its own would be one more packet in front of the frame's first graph. */
int lav_stage_many_block(int n, const void *const *src, float *const *dst, const int *dims, const long *strides, const int *src_is_u8,
                         const void *block, int block_bytes, void *block_dst, void *stream);

/* Small dense layer out[b][o] = act(bias[o] + sum_k weight[o][k] x[b][k]) (weight in nn.Linear layout [out][in], bias or NULL;
 * act 0 = none, 1 = sigmoid): the brake classifier nn.Sequential(Linear(1024, 1), Sigmoid) of team_code_v2/models/rgb.py:62,79. */
int lav_linear_act(const float *x, int batch, int in_features, const float *weight, const float *bias, int out_features,
                   int act, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * 6c. Fixed-capacity, device-resident "other vehicles" batch.  The reference reads every detection back
 *     to the host (team_code_v2/model_inference.py:101-108: up to ~120 scalar device->host syncs) and runs the others
 *     branch on a data-dependent batch (:123-187).  Here the count stays in HBM:
 *
 * lav_det_decode: from the peak rows of lav_extract_peaks ([ncls][max_det][7] = score, x, y, size0, size1, ori0, ori1) of
 *     class `cls`, keep a row when score > min_score, near_px < |(x,y) - (ego_x,ego_y)| < far_px and not
 *     max(size0,size1) < min_box (det_inference, model_inference.py:95-121), and |(x,y) - (cx,cy)| > skip_px (the ego's own
 *     box, :131-133); survivors, in score order, give actors[2 i], actors[2 i + 1] = ((x - cx)/ppm, (y - cy)/ppm) (ego-frame
 *     metres) and actors[2 max_det + i] = atan2(ori1, ori0); *n_out = their number.  Entries beyond it are zero.
 * lav_batch_limit: from now on the batch-aware launches enqueued BY THIS THREAD - lav_conv2d, lav_crop_rotate, lav_gru_cast -
 *     skip the rows (images, crops, samples) >= *d_rows, read on the device when the kernel runs: a capacity-sized batch
 *     costs what its live rows cost, with no host round trip in between.  Skipped rows of the outputs are left untouched.
 *     NULL switches it off.  (A pointer, not a value: the launches can be captured in a HIP graph.)
 * ------------------------------------------------------------------------------------------ */
int lav_det_decode(const float *rows, int ncls, int max_det, int cls, double min_score, double ego_x, double ego_y,
                   double near_px, double far_px, double min_box, double cx, double cy, double skip_px, double ppm,
                   float *actors, int *n_out, void *stream);
int lav_batch_limit(const int *d_rows);
/* lav_det_decode_report (ABI 28): lav_det_decode, and the same launch also writes the [ncls][max_det][7] peak rows to host_rows, the
 *     count to host_n and then increments *host_seq (system-scope release) - three pointers into pinned, device-mapped HOST memory
 *     (hipHostMalloc).  The reference reads every detection back to the host (model_inference.py:101-108); here the host polls
 *     host_seq instead of fetching rows and count with two device->host copies and an event between the heads and the others
 *     graph.  All three NULL = lav_det_decode. */
int lav_det_decode_report(const float *rows, int ncls, int max_det, int cls, double min_score, double ego_x, double ego_y,
                          double near_px, double far_px, double min_box, double cx, double cy, double skip_px, double ppm,
                          float *actors, int *n_out, float *host_rows, int *host_n, unsigned *host_seq, void *stream);

/* ------------------------------------------------------------------------------------------
 * 7. Training-side pillar ops: what PointPillarNet needs in train mode, where BatchNorm1d uses batch
 *    statistics and therefore cannot be folded into the fused inference kernel.  They replace the two
 *    torch_scatter calls and coords.unique(dim=0) of lav/models/point_pillar.py:55-68, 81-85, 33 and give
 *    autograd what it needs (arg-max for the backward of scatter_max).
 *
 * lav_pillar_decorate: grid_locations + pillar_generation + decorate (point_pillar.py:55-85).
 *    points [batch][max_points][D]; outputs sized for the worst case (batch*max_points rows):
 *    unique_coords [P][3] = (cloud, xi, yi) sorted like torch.unique(dim=0); inverse [N_kept] pillar of each kept
 *    point; kept_src [N_kept] flat index (cloud*max_points + row) of each kept point - kept points stay in input
 *    order; decorated [N_kept][D+5] = (point, xyz - pillar mean, x - cell_x, y - cell_y) with the reference's swapped
 *    cell origin; counts [2] (device) = {P, N_kept}.  Pillar means are the same order-independent fixed-point sums as
 *    in lav_pillar_scatter.  Workspace: lav_pillar_decorate_workspace_bytes (no at-rest state; a lav_pillar_scatter workspace of
 *    the same geometry also serves and stays valid).  Any output except decorated/counts may be NULL.
 *
 * lav_scatter_max: out[s][c] = max over rows i with index[i] == s of src[i][c]; argmax[s][c] = the lowest such row
 *    (n for an empty segment, whose out is 0 - torch_scatter's convention).  src [n][channels], index [n] int32.
 * lav_scatter_max_backward: grad_src[argmax[s][c]][c] = grad_out[s][c], zero elsewhere.
 * ------------------------------------------------------------------------------------------ */
size_t lav_pillar_decorate_workspace_bytes(int batch, int max_points, const lav_grid *grid);
int lav_pillar_decorate(const float *points, const int *h_num_points, int batch, int max_points, int D,
                        const lav_grid *grid, int *unique_coords, int *inverse, int *kept_src, float *decorated,
                        int *counts, void *workspace, size_t workspace_bytes, void *stream);
int lav_scatter_max(const float *src, const int *index, int n, int channels, int num_segments, float *out, int *argmax,
                    void *stream);
int lav_scatter_max_backward(const float *grad_out, const int *argmax, int n, int channels, int num_segments,
                             float *grad_src, void *stream);

/* ------------------------------------------------------------------------------------------
 * 7b. Train-mode BatchNorm2d (batch statistics) with the neighbouring ReLU / residual add fused, forward and backward, NCHW
 *     float32.  Replaces the nn.BatchNorm2d + nn.ReLU (+ add) launches of the student networks in
 *     lav/lav_final_v2.py:140-259: ConvBackbone's Conv -> ReLU -> BatchNorm (team_code_v2/models/lidar.py:57-108; relu_pre)
 *     and ResNet-18's Conv -> BatchNorm (-> + identity) -> ReLU (lav/models/resnet.py; relu_post, residual).
 *
 *     forward:   t = relu_pre ? max(x, 0) : x;   mean/var over (batch, plane) per channel (biased var, float64 sums);
 *                y = (t - mean) / sqrt(var + eps) * gamma + beta (+ residual) (-> ReLU if relu_post)
 *                save_mean / save_var (biased) / save_rstd [channels] are written for the backward and the running statistics
 *                (the caller updates those: running = (1 - m) * running + m * (mean, var * n / (n - 1))).
 *     backward:  g = relu_post ? dy * [y > 0] : dy  (written to dres when the forward had a residual: that branch's gradient);
 *                dbeta = sum g, dgamma = sum g * xhat, dx = gamma * rstd * (g - dbeta / n - xhat * dgamma / n) (* [x > 0] if relu_pre)
 *     relu_pre excludes relu_post / residual.  y is only read when relu_post.  Two launches each way; sums are reduced in a
 *     fixed order (bit-reproducible).  workspace: lav_bn_train_workspace_bytes(channels) bytes, no at-rest state.
 * ------------------------------------------------------------------------------------------ */
size_t lav_bn_train_workspace_bytes(int channels);
int lav_bn_train_forward(const float *x, const float *residual, float *y, int batch, int channels, long plane, const float *gamma,
                         const float *beta, double eps, int relu_pre, int relu_post, float *save_mean, float *save_var,
                         float *save_rstd, void *workspace, size_t workspace_bytes, void *stream);
int lav_bn_train_backward(const float *x, const float *y, const float *dy, int batch, int channels, long plane, const float *gamma,
                          const float *save_mean, const float *save_rstd, int relu_pre, int relu_post, float *dx, float *dres,
                          float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream);
/* The same pair leaving the BOUND of what it writes (round 6): amax_y / amax_dx (device, lav_bn_train_amax_count floats, or NULL) receive
 * the largest finite |y| resp. |dx| of every workgroup of the normalising launch - in the training graph (lav/lav_final_v2.py:140-259)
 * the next convolution's input is a BatchNorm's output and a convolution's output gradient is a BatchNorm's input gradient, so that a
 * LAV_CONV_F16X3 step takes its scales from these parts (lav_conv2d_amax, lav_conv_wgrad_amax) instead of measuring every activation and
 * gradient tensor with a launch of its own (173 lav_absmax_parts launches per train_full step). */
int lav_bn_train_amax_count(int batch, int channels, long plane);
int lav_bn_train_forward_amax(const float *x, const float *residual, float *y, int batch, int channels, long plane, const float *gamma,
                              const float *beta, double eps, int relu_pre, int relu_post, float *save_mean, float *save_var,
                              float *save_rstd, float *amax_y, void *workspace, size_t workspace_bytes, void *stream);
int lav_bn_train_backward_amax(const float *x, const float *y, const float *dy, int batch, int channels, long plane, const float *gamma,
                               const float *save_mean, const float *save_rstd, int relu_pre, int relu_post, float *dx, float *dres,
                               float *dgamma, float *dbeta, float *amax_dx, void *workspace, size_t workspace_bytes, void *stream);

/* The same pair with Dropout2d's per-(sample, channel) multiplier (ABI 29): y = relu_post(chmask[b][c] * BN(x) + residual), and its backward
 * (the residual's gradient dres = the relu_post-masked dy, the normalisation's gradient chmask * dres).  chmask [batch][channels] on the
 * device ({0, 1 / (1 - p)}, drawn by the caller); relu_pre is not offered.  Two launches each way, sums in a fixed order, as above. */
int lav_bn_train_forward_mask(const float *x, const float *residual, const float *chmask, float *y, int batch, int channels, long plane,
                              const float *gamma, const float *beta, double eps, int relu_post, float *save_mean, float *save_var,
                              float *save_rstd, float *amax_y, void *workspace, size_t workspace_bytes, void *stream);
int lav_bn_train_backward_mask(const float *x, const float *y, const float *dy, const float *chmask, int batch, int channels, long plane,
                               const float *gamma, const float *save_mean, const float *save_rstd, int relu_post, float *dx, float *dres,
                               float *dgamma, float *dbeta, float *amax_dx, void *workspace, size_t workspace_bytes, void *stream);

/* Weight gradient of a 3x3, padding-1 convolution of stride 1 or 2, or of a 7x7, padding-3, stride-2 convolution (round 5): the weight half of torch.autograd's convolution backward for
 * the stage convolutions of ConvBackbone (team_code_v2/models/lidar.py:57-108) and the four heads' first convolutions (lidar.py:147-161)
 * inside LAV.train_lidar's backward (lav/lav_final_v2.py:140-259), which the reference runs on cuDNN (here: MIOpen's igemm_wrw).
 *     dw[co][ci][ky][kx] = sum over (n, y, x) of dy[n][co][y][x] * x[n][ci][stride y + ky - pad][stride x + kx - pad]      (zero padding, pad = ksize / 2)
 * x [batch][cin][h][w], dy [batch][cout][h / stride][w / stride], dw [cout][cin][ksize][ksize] (PyTorch layouts, float32, device, 16-byte
 * aligned); cin and cout multiples of 64, w a multiple of 4 (stride 2: h even, w a multiple of 8).  bf16x6 arithmetic on the matrix cores (operands split exactly into three bf16
 * pieces, six partial products, float32 accumulation), partial sums added in a fixed order: bit-reproducible.  The forward and the
 * data gradient of the same layers are lav_conv2d launches (the data gradient as the transposed convolution with the same weight
 * tensor); lav_amd/train/hipnn.py wires the three into one torch.autograd.Function.
 * workspace: lav_conv_wgrad_workspace_bytes (0 = shape not supported), private to the stream. */
size_t lav_conv_wgrad_workspace_bytes(int batch, int cin, int cout, int h, int w, int ksize, int stride);
int lav_conv_wgrad(const float *x, const float *dy, int batch, int cin, int cout, int h, int w, int ksize, int stride, float *dw,
                   void *workspace, size_t workspace_bytes, void *stream);
/* the same on TWO fp16 pieces per operand and three partial products (round 6, the weight-gradient side of LAV_CONV_F16X3): amax_x /
 * amax_dy (device, n_amax_* floats each) hold maxima of the finite |x| / |dy| in parts - lav_absmax_parts, or what lav_conv2d_amax
 * left - from which every task takes the two power-of-two scales; NULL, NULL: lav_conv_wgrad's bf16x6 arithmetic. */
int lav_conv_wgrad_amax(const float *x, const float *dy, int batch, int cin, int cout, int h, int w, int ksize, int stride, float *dw,
                        void *workspace, size_t workspace_bytes, const float *amax_x, int n_amax_x, const float *amax_dy, int n_amax_dy,
                        void *stream);

/* ------------------------------------------------------------------------------------------
 * 7c. Transposed convolutions with kernel == stride ("pointwise" up-convolutions, ABI 28): every output pixel has one contributing
 *     input pixel and tap, so the layer is k*k independent [cout x cin] x [cin x pixels] products - two of the BEV backbone's three
 *     up-convolutions (team_code_v2/models/lidar.py:114-131: ConvTranspose2d(64, 128, 1, 1) and ConvTranspose2d(128, 128, 4, 4, 1, 2),
 *     each + ReLU + eval BatchNorm into a slice of the 384-channel feature map):
 *     y[n][out_c_offset + co][k iy + ky - pad][k ix + kx - pad] = scale[co] * relu?(sum_ci w[ci][co][ky][kx] x[n][ci][iy][ix]) + shift[co];
 *     output positions without a contributing input pixel (output_padding) hold scale * relu?(0) + shift.  Exact fp32 products and
 *     accumulation on v_mfma_f32_32x32x2_f32.  Supported: k in {1, 4}, cin in {64, 128}, cout a multiple of 128 (k = 1) / 32 (k = 4),
 *     pad < k; k = 1 without padding.  x [batch][cin][ih][iw], y [batch][out_c_total][OH][OW], OH = (ih - 1) k - 2 pad + k + out_pad.
 *     lav_upconv_pointwise_pack repacks the PyTorch ConvTranspose2d weight [cin][cout][k][k] on the host
 *     (lav_upconv_pointwise_packed_floats floats).  amax_out (or NULL): lav_upconv_pointwise_parts floats, the largest finite |y| each
 *     workgroup wrote - what lav_conv2d_amax leaves for LAV_CONV_F16X3 readers of the feature map.
 * ------------------------------------------------------------------------------------------ */
size_t lav_upconv_pointwise_packed_floats(int cin, int cout, int k);
int lav_upconv_pointwise_pack(int cin, int cout, int k, const float *h_weight, float *h_packed);
int lav_upconv_pointwise_parts(int batch, int cin, int cout, int ih, int iw, int k, int pad, int out_pad);
int lav_upconv_pointwise(int batch, int cin, int cout, int ih, int iw, int k, int pad, int out_pad, const float *x, const float *w_packed,
                         const float *scale, const float *shift, int relu_pre, int out_c_total, int out_c_offset, float *y,
                         float *amax_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * 8. Two stacked 1-D convolutions in one launch - one half of ERFNet's non_bottleneck_1d block
 *    (lav/models/erfnet.py:45-56):  y = relu?( (conv1x3_dB( relu( conv3x1_dA(x) + bias_a ) ) + bias_b) * scale + shift
 *    + residual ).  x, y, residual [batch][channels][h][w] (same shape), stride 1, "same" padding (pad = dilation).
 *    One workgroup per image row; the intermediate stays in LDS.  Supported: w in {32, 64, 128},
 *    channels a multiple of 16 with ceil(channels/32) <= 128/w (ERFNet: 16@128, 64@64, 128@32).
 *    Weights: lav_conv1d_pair_pack_weights repacks a PyTorch [cout][cin][3] tensor (the unit kernel dimension
 *    squeezed) on the host into all the forms the kernels read - exact fp32, three bf16 pieces, two scaled fp16 pieces with
 *    their scale and the largest L1 norm of a filter behind them (round 6) -; scale/shift/residual may be NULL.
 * ------------------------------------------------------------------------------------------ */
size_t lav_conv1d_pair_packed_weight_floats(int channels);
int lav_conv1d_pair_pack_weights(int channels, const float *h_weight, float *h_packed);
/*
 * lav_conv1d_pair_chain: a RUN of such pairs over one map - the non_bottleneck_1d blocks of an ERFNet stage
 * (lav/models/erfnet.py:25-62: 5 blocks at 64 channels, 8 dilated ones at 128, 2 + 2 in the decoder) - as ONE persistent launch:
 * a workgroup per image row walks all pairs; between two pairs only its two neighbour rows (y -+ d_a) travel through memory
 * (write-through stores + a per-row progress counter), its own row, the block residual and the next pair's first weights never
 * leave the CU.  residual[i] != 0: pair i adds the INPUT of pair i-1 (the block's input) before its ReLU; the run starts at a
 * block boundary.  out[i]: output buffer of pair i ([batch][channels][h][w] each, all distinct; out[npairs-1] is the result).
 * batch * h must not exceed the CU count (every row's workgroup waits for its neighbours'); three bf16 pieces per operand (lav_conv1d_pair_chain_f16: two fp16 pieces).  Waits are
 * bounded: a workgroup that gives up raises the launch's abort word (its peers poll it and stop waiting too), fills ITS row of
 * out[npairs-1] with NaN - a voided launch cannot be mistaken for a result: every row of the output is either the complete result or
 * NaN (round 5) - and raises a sticky counter: lav_conv1d_pair_chain_status copies {workgroups that gave up, launches}
 * since the workspace was zero-filled (it SYNCHRONISES `stream`; 0 = every result was valid).
 * workspace: lav_conv1d_pair_chain_workspace_bytes (sticky counters | one progress counter per row, capacity rounded up to 64 rows | the fp16
 * runs' 16 x capacity count-and-maximum words), ZERO before its first use, private to the stream.
 */
size_t lav_conv1d_pair_chain_workspace_bytes(int batch, int h);
size_t lav_conv1d_pair_chain_lds_bytes(int channels, int w, int d_b_max);
int lav_conv1d_pair_chain(int batch, int channels, int h, int w, int npairs, const int *d_a, const int *d_b, const int *residual,
                          const int *relu_post, const float *x, const float *const *wa_packed, const float *const *bias_a,
                          const float *const *wb_packed, const float *const *bias_b, const float *const *scale,
                          const float *const *shift, float *const *out, void *workspace, size_t workspace_bytes, void *stream);
/* lav_conv1d_pair_chain_f16 (ABI 28): the same run, same arguments and contract, on TWO power-of-two-scaled fp16 pieces per operand and
 * three matrix products instead of three bf16 pieces and six (LAV_CONV_F16X3 for ERFNet's runs: half the matrix instructions, 2/3 of the
 * weight bytes a row streams per pair).  The weights' scale comes from lav_conv1d_pair_pack_weights (which packs all three forms); the
 * activations' scale is derived per workgroup and pair from the largest finite magnitude of the three rows it multiplies (the
 * neighbours' maxima travel IN the hand-off's flag: one 64-bit word {pairs done | row maximum} per pair and row), the intermediate row's from a bound (largest input x largest L1 norm of a filter +
 * largest |bias|).  Error: that of an fp32 dot product (tests/test_gpu_conv.py, against float64); not bit-identical to the bf16 run. */
int lav_conv1d_pair_chain_f16(int batch, int channels, int h, int w, int npairs, const int *d_a, const int *d_b, const int *residual,
                              const int *relu_post, const float *x, const float *const *wa_packed, const float *const *bias_a,
                              const float *const *wb_packed, const float *const *bias_b, const float *const *scale,
                              const float *const *shift, float *const *out, void *workspace, size_t workspace_bytes, void *stream);
/* lav_conv1d_pair_chain_region (ABI 28): several runs that follow each other on one stream share ONE cleaning of their progress counters.
 * The runs THIS THREAD enqueues from now on keep their counters at rows [row_offset, row_offset + batch * h) of the workspace's counter
 * array (capacity: what lav_conv1d_pair_chain_workspace_bytes was asked for, rounded up to 64 rows) and, in front of the run, zero the
 * first clean_rows counters of the array (clean_rows > 0: the first run of a sequence, for all of them), nothing (0: a launch earlier on the
 * stream cleaned this run's rows - each region is good for ONE run per cleaning), or their own rows (-1 with row_offset 0: the default,
 * one small launch in front of every run).  ERFNet's four runs per frame: one cleaning launch instead of four (lav/models/erfnet.py:109-131).
 * A pointer-free thread-local setting like lav_batch_limit: captured launches keep what was set when they were enqueued. */
int lav_conv1d_pair_chain_region(int row_offset, int clean_rows);
int lav_conv1d_pair_chain_status(const void *workspace, int *h_timeouts_launches2, void *stream);
size_t lav_conv1d_pair_lds_bytes(int channels, int w, int d_b);
/*
 * lav_conv3x3_run_f16 (ABI 31): a RUN of nlayers (<= 8) identical layers conv3x3(stride 1, pad 1, no bias) -> ReLU -> y * scale + shift at
 * 64 or 128 channels over one [channels][h][w] map (batch 1) as ONE persistent launch - the stages of the BEV backbone behind their
 * stride-2 layer (team_code_v2/models/lidar.py:57-108).  A workgroup owns one output row (and a slice of the output channels) for all
 * layers; between two layers the rows travel through two ping-pong maps of the workspace (write-through stores) and one 64-bit word
 * {layers done | largest finite |y| written} per workgroup and layer, the protocol of lav_conv1d_pair_chain_f16.  Arithmetic of
 * LAV_CONV_F16X3: two fp16 pieces per operand, three products, fp32 accumulate.  w_f16[i]: the fp16 section of layer i's packed weights
 * (lav_conv_pack_weights of a LAV_CONV_F16X3 layer, at lav_conv_f16_weights_offset floats).  The first layer's activation scale comes from
 * amax_in (amax_in_count maxima that bound |x|: lav_absmax_parts, or a producer's lav_conv2d_amax); inside the run every workgroup takes
 * it per layer from the words it waited for.  amax_out (optional): one float per workgroup (h * slices =
 * lav_conv3x3_run_f16_amax_count) - the maxima of the result, as lav_conv2d_amax leaves them.  Only the last layer's map is an output.
 * Waits are bounded (LAV_CHAIN_SPIN_LIMIT): a workgroup that gives up raises the launch's abort word (its peers stop waiting too), fills
 * its part of `out` with NaN and raises a sticky counter; lav_conv3x3_run_f16_status copies {workgroups that gave up, launches} since the
 * workspace was zero-filled (it SYNCHRONISES `stream`).  workspace: lav_conv3x3_run_f16_workspace_bytes (0: the geometry is not served -
 * run the layers one launch each), ZERO before its first use, private to the stream.
 */
size_t lav_conv3x3_run_f16_workspace_bytes(int channels, int h, int w, int nlayers);
size_t lav_conv3x3_run_f16_lds_bytes(int channels, int h, int w);
size_t lav_conv3x3_run_f16_weight_bytes(int channels);
int lav_conv3x3_run_f16_amax_count(int channels, int h, int w);
long lav_conv_f16_weights_offset(const lav_conv *c);
int lav_conv3x3_run_f16(int channels, int h, int w, int nlayers, const float *x, const void *const *w_f16, const float *const *scale,
                        const float *const *shift, float *out, const float *amax_in, int amax_in_count, float *amax_out, void *workspace,
                        size_t workspace_bytes, void *stream);
int lav_conv3x3_run_f16_status(const void *workspace, int *h_timeouts_launches2, void *stream);

/*
 * lav_conv3x3_tile_f16 (ABI 40): a run of nlayers (<= 3) of the same layers at 64 channels as ONE launch without any hand-off between
 * workgroups - stage s1 of the BEV backbone behind its stride-2 layer.  A workgroup owns an 8 x 16 output tile for all layers: it stages
 * the input tile with a halo of nlayers pixels once, keeps the intermediate maps in LDS and recomputes their halo.  Arithmetic, weights
 * (w_f16), scale / shift and amax_in as lav_conv3x3_run_f16; inside the run a workgroup takes a layer's activation scale from the largest
 * finite |value| of the region it just computed.  amax_out (optional): one float per workgroup (lav_conv3x3_tile_f16_amax_count) - the
 * maxima of the result, as lav_conv2d_amax leaves them.  No workspace, no waits: nothing to time out.  lav_conv3x3_tile_f16_lds_bytes
 * returns 0 where the geometry is not served (other channel counts, more layers): run the layers one launch each.  Any h, w >= 1.
 */
size_t lav_conv3x3_tile_f16_lds_bytes(int channels, int h, int w, int nlayers);
int lav_conv3x3_tile_f16_amax_count(int channels, int h, int w, int nlayers);
int lav_conv3x3_tile_f16(int channels, int h, int w, int nlayers, const float *x, const void *const *w_f16, const float *const *scale,
                         const float *const *shift, float *out, const float *amax_in, int amax_in_count, float *amax_out, void *stream);
int lav_conv1d_pair(int batch, int channels, int h, int w, int d_a, int d_b, const float *x, const float *wa_packed,
                    const float *bias_a, const float *wb_packed, const float *bias_b, const float *scale, const float *shift,
                    const float *residual, int relu_post, float *y, void *stream);

/* 2x2/stride-2 max pooling + per-channel affine (+ ReLU) written into a channel window of y: the pooled branch of
 * ERFNet's DownsamplerBlock, cat([conv(x), pool(x)]) -> BatchNorm -> ReLU (lav/models/erfnet.py:9-23), whose
 * convolution branch is lav_conv2d writing the other window of the same tensor.
 * x [batch][channels][h][w] (h, w even); y [batch][out_c_total][h/2][w/2]. */
int lav_pool_affine(const float *x, int batch, int channels, int h, int w, const float *scale, const float *shift, int relu,
                    float *y, int out_c_total, int out_c_offset, void *stream);

/* ERFNet's two entry DownsamplerBlocks (3 -> 16 -> 64 channels) as one launch (ABI 47; csrc/erfnet_edge.hip):
 *     y = block2(block1(x)),   block(x) = relu(bn(cat(conv3x3/s2(x), maxpool2x2(x))))
 * x [batch][3][h][w] raw input (h, w multiples of 4); y [batch][64][h/4][w/4].  Block 1 as DownsamplerBlock.engine folds it:
 * w1 [13][3][3][3] and b1 [13] with the input affine folded in, pad_value what out-of-image taps of block 1 read (-t/s; 0 without
 * an input affine), scale1 / shift1 [16]: the BatchNorm affine of the 13 convolution channels, then that of the 3 pooled
 * channels with the input affine folded in.  Block 2: w2 [48][16][3][3] (16-byte aligned), b2 [48], scale2 / shift2 [64]
 * (48 convolution channels, then 16 pooled).  Both convolutions are fp32 FMA chains (block 2 on v_mfma_f32_16x16x4_f32): the
 * result does not depend on LAV_CONV_PRECISION.  No workspace. */
int lav_erfnet_entry(const float *x, int batch, int h, int w, const float *w1, const float *b1, float pad_value, const float *scale1,
                     const float *shift1, const float *w2, const float *b2, const float *scale2, const float *shift2, float *y,
                     void *stream);

/* ------------------------------------------------------------------------------------------
 * Train mode of ERFNet's factorised convolution pairs (ABI 29; csrc/conv_pair_train.hip): one pair of a non_bottleneck_1d is
 *     t = relu(conv3x1_d(x) + ba),   z = conv1x3_d(t) + bb          (padding d, dilation d along the kernel's axis)
 * x, t, z [batch][channels][h][w]; wa = conv3x1.weight [channels][channels][3][1], wb = conv1x3.weight [channels][channels][1][3]
 * (PyTorch layouts, no repack), ba / bb [channels].  (channels, w) in {(16, 128), (64, 64), (128, 32)} (lav_pair_train_supported),
 * any batch and h.  float32 FMA arithmetic; every sum in a fixed order, no atomics: bit-reproducible.
 *     forward:  one launch; writes t (for the backward) and z.
 *     backward: dt = [t > 0] * conv1x3_d^T(dz) (written to dt, scratch of x's size), dx = conv3x1_d^T(dt),
 *               dwb / dbb from (dz, t), dwa / dba from (dt, x): per-row-group partial sums in the workspace
 *               (lav_pair_train_workspace_bytes) reduced in group order.  Six launches.
 * ------------------------------------------------------------------------------------------ */
int lav_pair_train_supported(int channels, int width);
size_t lav_pair_train_workspace_bytes(int batch, int channels, int h);
int lav_pair_train_forward(const float *x, const float *wa, const float *ba, const float *wb, const float *bb, int batch, int channels,
                           int h, int w, int dil, float *t, float *z, void *stream);
int lav_pair_train_backward(const float *x, const float *t, const float *dz, const float *wa, const float *wb, int batch, int channels,
                            int h, int w, int dil, float *dt, float *dx, float *dwa, float *dba, float *dwb, float *dbb, void *workspace,
                            size_t workspace_bytes, void *stream);

/* Pixel-wise softmax cross-entropy with mean reduction, F.cross_entropy(logits [batch][classes][plane], labels [batch][plane] int64)
 * for classes <= 8 (ABI 29): loss[0] (device float) = mean over batch * plane of logsumexp - logit[label], dlogits = (softmax - onehot) /
 * (batch * plane).  Per-workgroup float64 partials summed in a fixed order by a second launch.  Labels must lie in [0, classes): the
 * launch does not check them (F.cross_entropy raises on others; here such a pixel would only be kept from reading past its classes -
 * it adds no loss but still counts in the mean).  lav_amd.train.hipnn.seg_cross_entropy checks the range before the launch.
 * workspace: lav_seg_xent_workspace_bytes() bytes. */
size_t lav_seg_xent_workspace_bytes(void);
int lav_seg_xent_forward(const float *logits, const long long *labels, int batch, int classes, long plane, float *loss, float *dlogits,
                         void *workspace, size_t workspace_bytes, void *stream);

/* The same loss on nearest-upsampled logits (ABI 30): F.cross_entropy(F.interpolate(logits, scale_factor=scale), labels) for
 * logits [batch][classes][h][w] (classes <= 8) and labels [batch][scale*h][scale*w] of label_bytes 1 (uint8) or 8 (int64), without
 * the upsampled map: per low-resolution cell, from the label histogram cnt of its scale x scale block, loss += s^2 lse - sum_k cnt_k
 * logit_k and dlogits = (s^2 softmax - cnt) / (batch s^2 h w).  Same partials, workspace and label contract as lav_seg_xent_forward
 * (lav_amd.train.hipnn.seg_cross_entropy_up checks labels and shapes before the launch). */
int lav_seg_xent_up_forward(const float *logits, const void *labels, int label_bytes, int batch, int classes, int h, int w, int scale,
                            float *loss, float *dlogits, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Offline point painting (ABI 32): the data collector's painter, lav/data_paint.py + lav/utils/point_painting.py, for a batch
 * of recorded frames in one launch.  Unlike lav_paint (the agent's painter: float32 projection, <= 4 cameras, fused rows) it
 * projects in FLOAT64 like CoordConverter.lidar_to_cam and writes only the class scores.
 * ------------------------------------------------------------------------------------------ */
typedef struct lav_camera_f64 {
    double l2w[16]; /* row-major 4x4 lidar_to_world  (point_painting.py:14-16) */
    double w2c[16]; /* row-major 4x4 world_to_cam    (:18-21) */
    double K[9];    /* row-major 3x3 intrinsics      (:7-12) */
} lav_camera_f64;

/*
 * lidar    [total][lidar_dim] float32: `frames` ragged clouds one after the other (xyz in columns 0..2; lidar_dim >= 3)
 * offsets  DEVICE int32 [frames + 1]: frame f owns rows offsets[f] .. offsets[f+1]-1; offsets[0] = 0, offsets[frames] = total,
 *          non-decreasing (1 <= frames <= 1024).  A row is painted from the last frame whose offset is <= its index, clamped to
 *          [0, frames-1]: wrong offsets give wrong values, never an access outside sem.
 * sem      [frames][ncam][sem_c+1][h][w] float32 class probabilities; channel 0 is the background.  1 <= ncam <= 8, sem_c == 4.
 * h_cams   ncam HOST records, copied into the kernel arguments.
 * painted  out [total][sem_c] (16-byte aligned).  xyz promoted to double; world = l2w.[x y z 1], cam = w2c.world,
 *          (X,Y,Z) = (cam_y, -cam_z, cam_x), p = K.(X,Y,Z), every product and sum rounded separately in k order;
 *          u = trunc(p0/(1e-5+p2)), v = trunc(p1/(1e-5+p2)), d = trunc(p2) as int64 (non-finite / out of range: invalid, numpy's
 *          astype(int) gives INT64_MIN there).  Per camera in order (later cameras overwrite), for d>=0, 0<=u<w, 0<=v<h:
 *          painted[c] = sem[1+c][v][u] * (1 - sem[0][v][u]) (float32 subtraction, float32 product); rows no camera sees are 0.
 *          Every row is written exactly once.
 * uvz      optional out [ncam][total][3] int32: (u, v, d) saturated to the int32 range, INT32_MIN where invalid; NULL to skip.
 */
int lav_paint_frames(const float *lidar, const int *offsets, int frames, int total, int lidar_dim, const float *sem, int ncam,
                     int sem_c, int h, int w, const lav_camera_f64 *h_cams, float *painted, int *uvz, void *stream);

/* img [n][h][w][c_src] uint8 (c_src 3 or 4) -> out [n][3][h][w] float32 of channels 0, 1, 2 (reverse != 0: 2, 1, 0 - BGR(A) ->
 * RGB, point_paint_dataset.py:32).  Exact. */
int lav_image_u8_to_f32(const unsigned char *img, int n, int h, int w, int c_src, int reverse, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Image augmentation for the camera trainers (ABI 33): the reference's augment(0.5) (lav/utils/augmenter.py: seven imgaug
 * operations in random order, each with probability 0.5) restated as this library's own specification - parity with imgaug is
 * UNPINNED (no imgaug, no recorded outputs); what is pinned is this kernel against lav_amd.data.augment.augment_numpy.
 * One record per image, drawn on the host (lav_amd.data.augment.Augmenter.draw).  32 four-byte words.
 * ------------------------------------------------------------------------------------------ */
enum { LAV_AUG_BLUR = 0, LAV_AUG_NOISE = 1, LAV_AUG_DROPOUT = 2, LAV_AUG_MULTIPLY = 3, LAV_AUG_CONTRAST = 4, LAV_AUG_GRAYSCALE = 5,
       LAV_AUG_ELASTIC = 6, LAV_AUG_OPS = 7 };

typedef struct lav_augment_params {
    int order[7];          /* the ops in execution order; a permutation of 0..6 (a repeated neighbourhood op or another id is skipped) */
    int active;            /* bit op: that op runs */
    int per_channel;       /* bit LAV_AUG_NOISE / LAV_AUG_DROPOUT: one random draw per pixel-channel instead of per pixel */
    unsigned sample;       /* Philox counter word 2: the sample id */
    unsigned tag;          /* Philox counter word 3 is tag | op << 8 | draw index; the stream tag sits in bits 16..31 */
    float blur_sigma;      /* informational (the kernel reads blur_w) */
    float blur_w[5];       /* normalised 5-tap Gaussian, computed in float64 on the host */
    float noise_scale;
    float dropout_p;
    float multiply[3];     /* per channel (three equal values when not per_channel) */
    float contrast[3];
    float gray_alpha;
    float elastic_alpha;
    float field_w[5];      /* the 5-tap Gaussian at sigma = 0.25 that smooths the displacement field */
} lav_augment_params;

/*
 * in, out  [n][h][w][3] uint8 (HWC, RGB), in != out and not overlapping (halos are read from `in`); h, w >= 1.
 * params   DEVICE array of n records.  seed: the Philox4x32-10 key (low word, high word); the counter of a pixel's random words is
 *          (x, y, params.sample, params.tag | op << 8 | draw), so they depend on the global pixel only, never on tile or launch shape;
 *          uniforms are (word >> 8) * 2^-24.
 * Every op maps uint8 to uint8: float32 arithmetic, every product and sum rounded separately in a fixed order, round-half-to-even
 * and clip to [0, 255] after the op.
 *   blur       separable 5-tap (horizontal, then vertical; float32 in between), border reflect-101
 *   noise      v + scale z,  z = sqrtf(-2 logf(u1)) cosf(2 pi u2), u1 = ((word >> 8) + 1) 2^-24; draw 0 words 0,1 (all channels, or
 *              channel 0) and 2,3 (channel 1), draw 1 words 0,1 (channel 2)
 *   dropout    0 where u < p (draw 0 word c of channel c; word 0 for all when not per_channel)
 *   multiply   v m[c]                contrast   128 + a[c] (v - 128)      (these two in float64, where they are exact)
 *   grayscale  g = (4899 R + 9617 G + 1868 B + 8192) >> 14;  v + alpha (g - v)
 *   elastic    raw field (dx, dy) = 2u - 1 from draw 0 words 0, 1 of every pixel; smoothed by field_w like blur (reflect-101), times
 *              alpha; out(x, y) = Keys bicubic (a = -0.75) of the image at (x - dx, y - dy), rows then columns, taps outside the image 0
 * The whole chain of an image runs in ONE launch: a workgroup owns a 64 x 32 output tile, loads it with a halo of 8 into LDS and
 * runs the active ops between two LDS buffers (blur consumes 2 of the halo, elastic 6: |displacement| <= 3.5 plus the cubic
 * footprint); pointwise ops are recomputed in the halo.  Wrong records give wrong pixels, never an access outside in / out / LDS.
 */
int lav_augment_u8(const unsigned char *in, unsigned char *out, int n, int h, int w, const lav_augment_params *params,
                   unsigned long long seed, void *stream);

/* ------------------------------------------------------------------------------------------
 * The data loaders' BEV map stacks behind the upload (ABI 34; train_bev_v2 / train_full_v2 --bev-on-device).  Every BEV plane of
 * every loader (lav/utils/datasets/{bev,temporal_bev,lidar,lidar_painted,temporal_lidar_painted}_dataset.py) is
 *     out = ( W2( crop( W1(src) ) ) > 0 )
 * W1, W2: cv2.warpAffine(INTER_LINEAR, constant border 0) on 8-bit images as lav_amd/data/image.py:warp_inverse_linear restates its
 * fixed-point path; crop(I)[r][c] = I[r + shift[0]][c + shift[1]], zero where that leaves the image.  Parity with OpenCV itself is
 * UNPINNED (as for the restatement); pinned, bit for bit, is this kernel against lav_amd.data.bev_stack.bev_stack_numpy.
 *
 * planes  [n][h][w] uint8, the decoded source planes; out [n][h][w] uint8, not overlapping planes; h, w >= 1 (any size).
 * coef    DEVICE [n][12] float64: the inverse map i00, i01, i10, i11, b1, b2 of W1, then of W2 - output pixel (x, y) samples
 *         (i00 x + i01 y + b1, i10 x + i11 y + b2).  Computed on the host (lav_amd.data.image.inverse_map): the device evaluates no
 *         trigonometric function and no division.  Finite, and no map may reach beyond +-2^30 pixels.
 * shift   DEVICE [n][2] int32: rows, columns.
 * threshold != 0: out = value > 0 (0 / 1); 0: the interpolated value.
 * Per warp, in float64 with every product and sum rounded on its own: X = rint((i00 x) 1024) + rint((i01 y + b1) 1024) + 16 (Y alike
 * from i10, i11, b2) as 64-bit integers; sx = clamp(X >> 10, -32768, 32767), fx = (X >> 5) & 31; the four taps (sy, sx) .. (sy + 1,
 * sx + 1), zero outside the image, with weights (32 - fy)(32 - fx) 32, (32 - fy) fx 32, fy (32 - fx) 32, fy fx 32; (sum + 2^14) >> 15.
 * One launch for all n planes; a workgroup owns a 64 x 32 tile and keeps the tile's footprint of W1(src) in LDS (it never reaches HBM);
 * a tile whose footprints exceed the LDS budget (8 KiB of W1(src), 16 KiB of src: no rotation does, a map that shrinks the image can)
 * interpolates every pixel from global memory instead.  Wrong records give wrong pixels, never an access outside planes / out / LDS.
 */
int lav_bev_stack_u8(const unsigned char *planes, const double *coef, const int *shift, unsigned char *out, int n, int h, int w,
                     int threshold, void *stream);
/* The launcher's rule, on the host: how many of one plane's tiles are zero without reading anything (counts[0]), staged in LDS
 * (counts[1]) and interpolated from global memory (counts[2]).  coef [12] and shift [2] are HOST pointers here.  No device needed. */
int lav_bev_stack_tile_paths(const double *coef, const int *shift, int h, int w, int *counts);

/* ------------------------------------------------------------------------------------------
 * The agent's per-tick debug frame (ABI 35; team_code_v2/lav_agent_fast.py:459-518, 567-581), rendered on the device: the cameras and
 * the telephoto image resized to the LiDAR panel's height, the LiDAR bird's-eye histogram (lidar_to_bev) with the drawing records on
 * it, the predicted BEV - side by side as a canvas of x_bins rows and w_rgb + w_tel + y_bins + bev_w columns that exists only tile by
 * tile in LDS - resized to half its size, with four lines of text.  Specification: lav_amd.agent.debug_view.compose_numpy, bit for
 * bit.  Parity with OpenCV's rasterisers, its resize and its font is UNPINNED (see there).
 *
 * rgb [rgb_h][rgb_w][3], tel [tel_h][tel_w][3] uint8 RGB; cloud [npts][stride] float32, x and y first (rows with a non-finite x or y
 * and rows outside the grid count nowhere); bev [3][x_bins][bev_w] float32, already sigmoided.
 * prims   DEVICE [nprims] records of 8 int32: kind (0 dot, 1 segment), x0, y0, x1, y1, radius, colour (r | g << 8 | b << 16), unused;
 *         LiDAR-panel pixel coordinates within +-2^20, in drawing order - a pixel takes the last record that covers it.  A dot
 *         covers dx^2 + dy^2 <= radius^2, a segment the pixels whose centre lies within distance 1 of it (and within radius of its
 *         bounding box).
 * text    DEVICE [4][text_len] uint8, 7-bit characters; font DEVICE [128][7] uint8, 5 x 7 glyphs, bit 4 the leftmost pixel; line l
 *         has its baseline-left at (4, 10 + 10 l), glyphs 6 pixels apart, white.
 * lut     DEVICE [11] uint8: grey of a cell holding 0 .. 10 (or more) points.
 * tables  DEVICE, 16-byte aligned, rows (i0, i1, w0, w1) int32 of lav_amd.data.image.resize_linear_table for, in this order: the
 *         camera panel's w_rgb columns, the telephoto panel's w_tel columns, the x_bins rows of each, the frame's columns and rows.
 *         Indices are clamped on the device: a wrong table gives wrong pixels, never an access outside the images or LDS.
 * The histogram's edges are np.linspace(start, stop, bins + 1) per axis, binned in float64 by np.histogramdd's rule.
 * counts  DEVICE workspace [x_bins][y_bins] uint32, zeroed here.  out [x_bins / 2][(canvas columns) / 2][3] uint8.
 * Up to three operations on `stream`: the zeroing, one launch over the cloud, one over the frame's 32 x 16 tiles.
 */
int lav_debug_view(const unsigned char *rgb, int rgb_h, int rgb_w, const unsigned char *tel, int tel_h, int tel_w, const float *cloud,
                   int npts, int stride, const float *bev, int bev_w, const void *prims, int nprims, const unsigned char *text,
                   int text_len, const unsigned char *font, const unsigned char *lut, const int *tables, double x_start, double x_stop,
                   int x_bins, double y_start, double y_stop, int y_bins, int w_rgb, int w_tel, unsigned *counts, unsigned char *out,
                   void *stream);

/* ------------------------------------------------------------------------------------------
 * The trainers' visual logs (ABI 36; lav/utils/logger.py: log_bev_info, log_lidar_info, log_seg_info, log_bra_info), composed on the
 * device from tensors a logged step left in HBM.  Specification: lav_amd.train.log_view.log_view_numpy, bit for bit.  Parity with
 * matplotlib's rasterisation and figure scaling, its font and imshow's normalisation is UNPINNED (see there).
 *
 * panels  DEVICE [npanels <= 8] records of 16 int32: kind, x, y, w, h (the rectangle in the frame; the source has w x h pixels), channels,
 *         colour (r | g << 8 | b << 16), palette offset, palette entries, bytes per label (1, 4 or 8), source address (low, high word),
 *         4 unused.  Kinds: 0 image [h][w][3] uint8; 1 labels [h][w] integers, label i + 1 -> palette[offset + i], the rest black;
 *         2 logits [channels][h][w] float32, np.argmax over the channels (first maximum, a NaN counts as one), then as labels;
 *         3 planes [channels][h][w] float32, grey floor((m - lo) * 255 / (hi - lo)) of the float64 channel mean m (sum in channel order
 *         over the count), lo / hi the smallest / largest finite mean of the panel; 0 where hi == lo or m is not finite; 4 the colour.
 *         A pixel takes the last panel that holds it, black where none does.
 * prims   DEVICE [nprims] records of 16 int32: kind (0 dot, 1 segment, 2 filled convex polygon), x0, y0, x1, y1, radius, colour, panel,
 *         x2, y2, x3, y3, vertices (3 or 4; a triangle repeats its last vertex), 3 unused.  Coordinates of the named panel, within
 *         +-2^20, in drawing order: a pixel takes the last record that covers it, and a record covers pixels of its panel's rectangle
 *         only.  Dots and segments as lav_debug_view; a polygon covers the pixels of its bounding box for which every int64 edge
 *         function is >= 0 or every one is <= 0.
 * text    DEVICE [nrows][text_len] uint8, 7-bit characters; origins DEVICE [nrows][2] int32 (x, y) baseline-left of each row; font
 *         DEVICE [128][7] uint8, 5 x 7 glyphs, bit 4 the leftmost pixel; glyphs 6 pixels apart, white, clipped to the frame.
 * palette DEVICE [npalette][3] uint8.  minmax DEVICE workspace of 16 uint64, zeroed here.  out [frame_h][frame_w][3] uint8.
 * Up to three operations on `stream`: the zeroing, one launch over the planes panels, one over the frame's 32 x 8 tiles.  Sizes and
 * indices of the tables are checked or clamped on the device; the sources' extents are the caller's word (lav_amd.ops.log_view checks
 * them against the tensors).
 */
int lav_log_view(const void *panels, int npanels, const void *prims, int nprims, const unsigned char *text, const int *origins, int nrows,
                 int text_len, const unsigned char *font, const unsigned char *palette, int npalette, unsigned long long *minmax,
                 int frame_h, int frame_w, unsigned char *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Open-loop metrics of one evaluated frame (ABI 37; eval_full_v2.py, lav_amd.train.evaluate), ADDED into an int64 accumulator that stays
 * in HBM: one launch per frame, nothing is copied to the host.  Specification: lav_amd.train.evaluate.eval_frame_numpy, bit for bit -
 * every counter is an integer and the distance sums add distances already quantised to 2^-20 m, so a route's result does not depend on
 * any order.  The reference has no evaluator: the definitions are this project's, parity with a reference is UNPINNED.
 *
 * The accumulator has 41 + 4 nbins words, as the size function says: frames; seg [3 channels][tp, fp, fn]; n_gt [2 classes];
 * det [2][tp, fp] at det_score; plan [6 commands][frames, sum of q, final q]; plan_nonfinite; others: matched, unmatched, nonfinite,
 * sum of the best mode's, of the top mode's, of the top mode's final q; hist [2][tp, fp][nbins].  The size function returns 0 for
 * nbins outside 1 .. 1024.
 *
 * pred_bev [3][h][w] float32 probabilities, labels [3][h][w] uint8 (the first planes of the loaders' BEV stack; non-zero = set), mask
 *         [h][w] uint8: per channel the pixels with a non-zero mask are counted as pred & label, pred & ~label, ~pred & label,
 *         pred = pred_bev > threshold.
 * rows    [2][max_det <= 32][7] as lav_extract_peaks leaves them.  Per class, in order, a row with (double)score > min_score takes the
 *         nearest free ground-truth actor of its class (squared pixel distance in float64, ties to the lowest index) if that lies within
 *         radius_px: a true positive, else a false positive; both go to hist bin min(nbins - 1, (int)(score * nbins)) and, where
 *         (double)score > det_score, to det.  Ground truth: locs [max_objs <= 64][num_plan + 1][2] float32 metres, typs [max_objs]
 *         int32, the first num_objs of them; pixel = (double)loc * ppm + centre of frame 0, actors outside [0, w) x [0, h) are ignored,
 *         n_gt counts the others.
 * ego_plan [num_plan <= 64][2] against ego_locs [num_plan + 1][2] from index 1: q_t = llrint(sqrt(dx^2 + dy^2) * 2^20) in float64; a
 *         plan with a distance that is not below 2^32 m (NaN, Inf) counts in plan_nonfinite only.  cmd in 0 .. 5.
 * other_cast [num_others <= max_det][6][num_plan][2], other_cmds [num_others][6], other_row [num_others] int32: the row of class 1
 *         each forecast came from.  A forecast of a row that took actor g is compared with locs[g] from index 1: S_m the sum of mode m's
 *         q_t, the best mode's S, the S and the final q of the first maximum of other_cmds (a NaN counts as one); the forecast of a
 *         false positive (or of a row outside the table) counts as unmatched, one with a non-finite distance as nonfinite.  All three
 *         may be NULL when num_others is 0.
 * Workgroups but the last count the segmentation, the last one does the rest; one 64-bit atomic per workgroup and counter.
 */
size_t lav_eval_acc_words(int nbins);
int lav_eval_frame(const float *pred_bev, const unsigned char *labels, const unsigned char *mask, int h, int w, float threshold,
                   const float *rows, int max_det, const float *locs, const int *typs, int max_objs, int num_objs, int num_plan,
                   const float *ego_plan, const float *ego_locs, int cmd, const float *other_cast, const float *other_cmds,
                   const int *other_row, int num_others, double ppm, double centre_x, double centre_y, double radius_px,
                   double min_score, double det_score, int nbins, long long *acc, void *stream);

/* ------------------------------------------------------------------------------------------
 * Held-out metrics of the camera checkpoints (ABI 38; eval_seg.py, eval_bra_v2.py, lav_amd.train.evaluate_camera).  Each call is one
 * launch on `stream` that ADDS integers into a caller-owned section of 64-bit words in HBM; nothing is copied to the host.
 * Specifications: lav_amd.train.evaluate_camera.eval_seg_numpy / eval_scores_numpy, word for word.  The reference has no evaluator:
 * the definitions are this project's, parity with a reference is UNPINNED.
 *
 * lav_eval_seg: the confusion matrix of labels [n][h scale][w scale] uint8 against logits [n][k][h][w] float32, 2 <= k <= 8, scale in
 *         {1, 2, 4, 8}: label pixel (y, x) is judged by logit pixel (y / scale, x / scale) - F.interpolate(logits, scale_factor=scale)
 *         (nearest) followed by argmax, without the up-sampled logits.  The prediction of a logit pixel is the FIRST maximum of its k
 *         channels (p = 0; for c in 1 .. k - 1: if x[c] > x[p]: p = c).  A logit pixel with a channel that is not finite adds its
 *         scale^2 label pixels to `nonfinite` and to nothing else; otherwise a label >= k adds 1 to `ignored` and to nothing else.
 *         The section has 68 words whatever k is: images, pixels (label pixels seen), ignored, nonfinite, conf [8][8] (row = label,
 *         column = prediction).  n h w scale^2 must not exceed 2^31 (a workgroup counts in 32 bits before its 64-bit atomics).
 * lav_eval_scores: scores [n] float32 against flags [n] uint8, one workgroup.  The section has 6 + 2 nbins words, 1 <= nbins <= 1024:
 *         samples, nonfinite, at [flag != 0][(double)score > threshold], hist [flag != 0][bin] with
 *         bin = clamp((int)(score * (float)nbins), 0, nbins - 1) in float32 (lav_eval_frame's rule).  A NaN or infinite score counts in
 *         samples and nonfinite only.
 */
int lav_eval_seg(const float *logits, const unsigned char *labels, int n, int k, int h, int w, int scale, unsigned long long *acc,
                 void *stream);
int lav_eval_scores(const float *scores, const unsigned char *flags, int n, double threshold, int nbins, unsigned long long *acc,
                    void *stream);

/* ------------------------------------------------------------------------------------------
 * Held-out metrics of the privileged BEV teacher (ABI 39; eval_bev_v2.py, lav_amd.train.evaluate_bev): one launch per LOADER BATCH on
 * `stream` that ADDS integers into an int64 accumulator in HBM; nothing is copied to the host.  Specification:
 * lav_amd.train.evaluate_bev.eval_plans_numpy, word for word.  The reference has no evaluator: the definitions are this project's,
 * parity with a reference is UNPINNED.
 *
 * ego_plan [batch][iters][6][num_plan][2], ego_cast [batch][6][num_plan][2], ego_cmds [batch][6], ego_locs [batch][num_plan + 1][2],
 * cmds [batch] int32, bras [batch] uint8 (non-zero = the frame brakes); other_cast [num_others][6][num_plan][2], other_cmds
 * [num_others][6], other_locs [num_others][num_plan][2] (each forecast's target in its vehicle's own frame), all three may be NULL when
 * num_others is 0.  batch >= 1, num_others >= 0, 1 <= num_plan <= 64, 1 <= iters <= 8.
 *
 * S = iters + 1 stages: stage 0 is ego_cast at the frame's command, stage s is ego_plan[.][s - 1] at the frame's command.
 * q_t = llrint(sqrt(dx^2 + dy^2) * 2^20) in float64, lav_eval_frame's rule.  The accumulator has 57 + 37 S words, as the size function
 * says (0 for iters outside 1 .. 8), in this order:
 *   frames; bad_cmd: frames whose command is outside 0 .. 5, which add to nothing else;
 *   plan [bra != 0][S][6 commands][frames, sum of q_t, q_{T-1}] against ego_locs[.][1 ..];
 *   plan_nonfinite [S]: a stage with a distance that is not below 2^32 m counts here and not in plan, every stage on its own;
 *   cmd_conf [command][first maximum of ego_cmds; a NaN counts as a maximum];
 *   others: forecasts scored; oth_nonfinite: forecasts with a non-finite distance in any mode, which add to nothing else;
 *   oth [4]: sums of the min mode's sum of q_t, of the top mode's, of the top mode's q_{T-1}, of the min mode's q_{T-1};
 *   oth_min_mode [6], oth_top_mode [6]: histograms of the mode with the smallest sum (the first minimum) and of the first maximum of
 *   other_cmds; oth_top_is_min: forecasts whose top mode is the min mode.
 * One wave per frame and per forecast, four to a workgroup; one 64-bit atomic per workgroup and counter.
 */
size_t lav_eval_plans_words(int iters);
int lav_eval_plans(const float *ego_plan, const float *ego_cast, const float *ego_cmds, const float *ego_locs, const int *cmds,
                   const unsigned char *bras, int batch, int iters, int num_plan, const float *other_cast, const float *other_cmds,
                   const float *other_locs, int num_others, long long *acc, void *stream);

/* ------------------------------------------------------------------------------------------
 * The LiDAR student beside the BEV teacher it was distilled from, on the same frames and the same crops (ABI 43; eval_distill_v2.py,
 * lav_amd.train.evaluate_distill): one launch per group of frames on `stream` that ADDS the PAIRED integers - what two separate
 * lav_eval_plans accumulators cannot give - into an int64 accumulator in HBM; nothing is copied to the host.  Specification:
 * lav_amd.train.evaluate_distill.eval_distill_numpy, word for word.  The reference has no evaluator: the definitions are this
 * project's, parity with a reference is UNPINNED.
 *
 * s_* the student's and t_* the teacher's outputs, lav_eval_plans' shapes: ego_plan [batch][iters][6][num_plan][2], ego_cast [batch][6]
 * [num_plan][2], ego_cmds [batch][6], other_cast [num_others][6][num_plan][2], other_cmds [num_others][6]; ego_locs [batch][num_plan + 1]
 * [2], cmds [batch] int32, other_locs [num_others][num_plan][2]; the five forecast tensors may be NULL when num_others is 0.  batch >= 1,
 * num_others >= 0, 1 <= num_plan <= 64, 1 <= iters <= 8.
 *
 * S = iters + 1 stages: stage 0 is the cast, stage s refinement s - 1 of the plan.  q_t = llrint(sqrt(dx^2 + dy^2) * 2^20) in float64,
 * lav_eval_frame's rule, and a path with a distance that is not below 2^32 m is non-finite; a score gap is llrint(|s - t| * 2^20) in
 * float64, non-finite where the difference is not below 2^32 (NaN, Inf).  The accumulator has 114 + 38 S words, as the size function says
 * (0 for iters outside 1 .. 8), in this order:
 *   frames; bad_cmd: frames whose command is outside 0 .. 5, which add to nothing else;
 *   ego_gap [S][6 modes][items, sum of q_t, q_{T-1}], the student's waypoints against the teacher's; ego_gap_nonfinite [S]: the
 *   non-finite (stage, mode) pairs, which count here instead;
 *   ego_closer [S][command][student, teacher, tie]: at the frame's command, whose sum of q_t against ego_locs[.][1 ..] is the smaller;
 *   ego_unjudged [S]: frames where either arm's is non-finite at that stage, which count here instead;
 *   cmd_agree [teacher's first maximum of ego_cmds][student's; a NaN counts as a maximum];
 *   cmd_gap [6 modes][items, sum of the score gaps]; cmd_nonfinite: the non-finite (frame, mode) gaps, which count here instead;
 *   others: forecasts scored; oth_nonfinite: forecasts with a non-finite path - either arm against other_locs or the student against
 *   the teacher, any mode - or a non-finite score gap, which add to nothing else;
 *   oth_gap [6 modes][sum of q_t, q_{T-1}], the student's forecast against the teacher's;
 *   oth_closer [student, teacher, tie] by each arm's smallest sum over its modes against other_locs, oth_closer_top [3] by the sum of
 *   each arm's own top mode (the first maximum of its other_cmds); oth_same_min: forecasts where both arms' min mode (the first
 *   minimum) is the same; oth_top_agree [teacher's top mode][student's]; oth_cmd_gap [6 modes]: sums of the score gaps.
 * One wave per frame and per forecast, four to a workgroup; one 64-bit atomic per workgroup and counter.
 */
size_t lav_eval_distill_words(int iters);
int lav_eval_distill(const float *s_ego_plan, const float *s_ego_cast, const float *s_ego_cmds, const float *t_ego_plan,
                     const float *t_ego_cast, const float *t_ego_cmds, const float *ego_locs, const int *cmds, int batch, int iters,
                     int num_plan, const float *s_other_cast, const float *s_other_cmds, const float *t_other_cast,
                     const float *t_other_cmds, const float *other_locs, int num_others, long long *acc, void *stream);

/* ------------------------------------------------------------------------------------------
 * Rotated-box metrics of one evaluated frame's detections (ABI 45; eval_det_v2.py, lav_amd.train.evaluate_det): one launch of one
 * workgroup on `stream` that ADDS integers into an int64 accumulator in HBM; nothing is copied to the host.  Specification:
 * lav_amd.train.evaluate_det.eval_det_numpy, word for word, which has the definitions in full and the final word on the order of every
 * operation.  The reference has no evaluator: the definitions are this project's, parity is UNPINNED.
 *
 * rows [2][max_det <= 32][7] = (score, x, y, w, h, cos, sin) as lav_extract_peaks / lav_heads_at_peaks leave them; locs [max_objs <= 64]
 * [num_plan + 1][2] of which frame 0 is read, typs [max_objs] int32, the first num_objs count (both may be NULL when num_objs is 0);
 * size_map, ori_map [2][h][w]: the loader's regression targets, from which actor g's box is read at (min(w - 1, int(px + 0.5)), iy
 * likewise), (px, py) = (double)loc * ppm + centre, kept when inside [0, w) x [0, h).  iou_q [num_iou <= 3] = llrint(threshold 2^20) in
 * 1 .. 2^20, range2 [num_range <= 3] = (edge ppm)^2 in squared pixels, heading_cos [num_heading <= 7] = cos(edge): HOST arrays, read
 * before the launch.  1 <= nbins <= 1024, min_score >= 0.
 *
 * A box (C, w, h, c, s) is valid when all are finite, w > 0, h > 0 and c c + s s is finite and > 0; its corners are C -+ w u -+ h v with
 * u = (s^, -c^), v = (c^, s^) the normalised direction, counter-clockwise.  iou_q(P, G) = llrint(IoU 2^20), at most 2^20, by clipping
 * P's corners against G's four edges (Sutherland-Hodgman, at most 8 vertices); 0 where a box is invalid.  Float64, + - * /, sqrt and
 * comparisons only.  Per class, rows with (double)score > min_score in order, four arms with their own taken sets: arm 0 takes the
 * nearest free actor within radius_px (lav_eval_frame's rule), arm 1 + k the free actor with the largest iou_q if that is >= iou_q[k]
 * and > 0; ties to the lowest index.  The accumulator has 135 + 16 nbins words, as the size function says (0 for nbins outside
 * 1 .. 1024), in this order:
 *   frames; n_gt [class][range bin]; gt_invalid [class]: in-map actors whose gathered box is invalid (they still count in n_gt);
 *   pred_invalid [class]: rows above min_score whose box is invalid; det [arm][class][range bin][tp, fp] over (double)score > det_score,
 *   range bin = the number of edges with d2 >= range2, d2 from the centre to the matched actor (tp) or to the row (fp);
 *   pairs [class][range bin]: arm 0's true positives above det_score; pair_invalid [class]: those with an invalid box on either side,
 *   which add to nothing below; sum_centre, sum_dw, sum_dh [class][range bin]: llrint(min(v, 2^32) 2^20) of sqrt(d2) / ppm, |w_p - w_g|
 *   / ppm, |h_p - h_g| / ppm; sum_iou: iou_q; heading [class][8]: the number of edges with c^_p c^_g + s^_p s^_g < heading_cos (a NaN:
 *   num_heading); hist [arm][class][tp, fp][min(nbins - 1, (int)(score * (float)nbins))].
 * One wave per arm and class, one lane per actor; 64-bit LDS atomics, then one 64-bit vector atomic per counter that changed and per counted row.
 */
size_t lav_eval_det_words(int nbins);
int lav_eval_det(const float *rows, int max_det, const float *locs, const int *typs, int max_objs, int num_objs, int num_plan,
                 const float *size_map, const float *ori_map, int h, int w, double ppm, double centre_x, double centre_y, double radius_px,
                 double min_score, double det_score, const long long *iou_q, int num_iou, const double *range2, int num_range,
                 const double *heading_cos, int num_heading, int nbins, long long *acc, void *stream);

/* ------------------------------------------------------------------------------------------
 * Open-loop metrics of the agent's rule layer over one evaluated frame (ABI 42; eval_drive_v2.py, lav_amd.train.evaluate_drive): one
 * launch of one workgroup on `stream` that ADDS integers into an int64 accumulator in HBM; nothing is copied to the host.
 * Specification: lav_amd.train.evaluate_drive.eval_drive_numpy, word for word, which also has the definitions in full.  The reference
 * tuned these rules in closed-loop CARLA and has no evaluator: the definitions are this project's, parity is UNPINNED.
 *
 * ego_plan, ego_cast [num_plan][2] (the cast is the commanded mode), ego_locs [num_plan + 1][2]; other_cast [num_others <= 64][6]
 * [num_plan][2], other_cmds [num_others][6], both may be NULL when num_others is 0; locs [max_objs <= 64][num_plan + 1][2], typs
 * [max_objs] int32, of which the first num_objs count (both may be NULL when num_objs is 0).  2 <= num_plan <= 64, cmd in 0 .. 5, bra
 * (the expert's brake label) 0 or 1, aim = the agent's aim_point[cmd] < num_plan, 1 <= nbins <= 1024.  The rule parameters are those of
 * LAVAgent: brake_speed (metres per step), cmd_thresh, plan_collide's dist_static and dist_moving (metres), behind = 0.5
 * pixels_per_meter and ego_radius = 4 / pixels_per_meter (metres); finite, at most 1e6, and all but cmd_thresh and behind not negative.
 *
 * q(a, b) = llrint(|a - b| * 2^20) in float64, lav_eval_frame's rule; P(p) the sum of a path's num_plan - 1 step quanta; S =
 * llrint(brake_speed (num_plan - 1) 2^20), L(x) = llrint(x 2^20); slow(p) = P(p) < S.  The driven path wp is ego_cast for commands 4
 * and 5, else ego_plan.  A trajectory is static when P < S, and hits when min_t q(traj[t], wp[t]) < L(dist_static) - or L(dist_moving)
 * when it is not static.  The accumulator has 92 + 6 nbins words, as the size function says (0 for nbins outside 1 .. 1024), in this
 * order:
 *   frames; plan_nonfinite: frames with a step of wp or q(wp[aim], ego_locs[1 + aim]) not below 2^32 m, which add to nothing else;
 *   expert_nonfinite: frames with such a step in ego_locs[1 ..], which add nothing to expert, speed and aim;
 *   cause [bra][slow(wp) | static hit << 1 | moving hit << 2] over the forecasts: vehicle k is skipped when (double)other_cast[k][0][0][1]
 *   > behind, its mode m when (double)other_cmds[k][m] < cmd_thresh (a NaN score stays);
 *   gt_cause: the same over the tracks of type 1 but those with x^2 + y^2 <= ego_radius^2 at frame 0 or locs[g][1][1] > behind, traj =
 *   locs[g][1 ..];  collide_conf [any track hit][any forecast hit];  ped [bra][a track of type 0 within L(dist_static) of wp];
 *   expert [bra][slow(ego_locs[1 ..])];  speed [cmd][frames, P(wp), P(expert), |difference|];  aim [cmd][q(wp[aim], ego_locs[1 + aim]),
 *   llrint(|dx| 2^20)];  modes [considered, static, hits, nonfinite] (a mode with a step or a distance that is not finite cannot hit);
 *   vehicles_behind;  clear_none [bra][kind] and clear_hist [bra][kind][min(nbins - 1, C >> 17)], C the least min_t q over the
 *   considered finite modes of that kind (0 static, 1 moving), none without one;  speed_hist [bra][min(nbins - 1, (P(wp) / (num_plan -
 *   1)) >> 14)], which stands before clear_hist.
 * One wave per mode and per track, four waves in all; one 64-bit atomic per counter that changes.
 */
size_t lav_eval_drive_words(int nbins);
int lav_eval_drive(const float *ego_plan, const float *ego_cast, const float *ego_locs, int num_plan, int cmd, int bra, int aim,
                   const float *other_cast, const float *other_cmds, int num_others, const float *locs, const int *typs, int max_objs,
                   int num_objs, double brake_speed, double cmd_thresh, double dist_static, double dist_moving, double behind,
                   double ego_radius, int nbins, long long *acc, void *stream);

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG scans of RGB frames in HBM (ABI 41; the agent's MJPEG recording).  Specification: lav_amd.agent.mjpeg.scan_numpy,
 * byte for byte; the stream format (4:2:0, full-range BT.601 in fixed point, an integer matrix DCT, the Annex K tables, restart
 * intervals) is stated in that module.  All integer arithmetic.
 *
 * frames          DEVICE [n][h][row_stride bytes]: rows of w RGB pixels, uint8, row_stride >= 3 w.  1 <= n <= 4096, 1 <= h, w <= 16384.
 * quality_tables  DEVICE [800] int32, lav_amd.agent.mjpeg.device_tables(quality): [0, 128) the luma and chroma quantisers in natural
 *                 order, [128, 192) the DCT matrix, [192, 256) the zigzag order, [256, 288) code | length << 16 of the luma and chroma DC
 *                 categories, [288, 800) the same of the luma and chroma AC symbols.  Indices read from it are masked or clamped: a wrong
 *                 table gives a wrong stream, never an access outside the workspace or LDS.
 * restart_mcus    MCUs (16 x 16 pixels) per restart interval, 1 .. 10: one wave codes an interval, one lane a block.
 * scans_out       DEVICE [n][scan_stride bytes], scan_stride >= lav_jpeg_scan_capacity(h, w, restart_mcus): per frame the
 *                 entropy-coded data of every interval, stuffed, with RST(k mod 8) behind all but the last - what stands between SOS
 *                 and EOI.  Bytes past the frame's length are left as they were.
 * lengths_out     DEVICE [n] int32: the bytes of each frame's scan.
 * workspace       DEVICE, 256-byte aligned, lav_jpeg_workspace_bytes(n, h, w, restart_mcus) bytes; needs no initialisation.
 * lav_jpeg_scan_capacity: the most bytes a frame's scan can take (every block 1660 bits, every byte stuffed, the markers); equals
 * lav_amd.agent.mjpeg.scan_capacity.  Both size functions return 0 for arguments lav_jpeg_encode would refuse.
 * Three launches on `stream` for the whole batch (coefficients per MCU, entropy coding per interval, compaction per interval); no
 * host synchronisation, no dependency between workgroups of one launch.
 */
long long lav_jpeg_scan_capacity(int h, int w, int restart_mcus);
size_t lav_jpeg_workspace_bytes(int n, int h, int w, int restart_mcus);
int lav_jpeg_encode(const unsigned char *frames, int n, int h, int w, int row_stride, const int *quality_tables, int restart_mcus,
                    unsigned char *scans_out, long long scan_stride, int *lengths_out, void *workspace, size_t workspace_bytes,
                    void *stream);

/* ------------------------------------------------------------------------------------------
 * Multi-tensor gradient statistics and a guarded Adam step (ABI 46; lav_amd.train.optim.FusedAdam, the trainers' --fused-optim).
 * Specification: lav_amd.train.optim.fused_adam_numpy, equal in every stored bit; the float64 sum of squares alone is pinned by a
 * bound (n * 2^-53 relative), its order of summation is the library's.
 *
 * The work is cut into chunks of lav_optim_chunk() elements.  Every table lives in DEVICE memory and is only read:
 * table  [ntensors] rows in chunk order: p, g, m, v float32, dense, 4-byte aligned, numel >= 1 elements each; lr, beta1, beta2, eps of
 *        this tensor; `state`, the index of its words in `state` (no two rows of a table share one); `chunk0`, the chunks of the rows
 *        before it (row 0: 0).  total_chunks = the sum of ceil(numel / chunk) over the rows.
 * watch  [nwatch] rows of read-only float32 buffers that are scanned for values that are not finite (BatchNorm's running statistics);
 *        chunk0 and watch_chunks as above.  May be null with nwatch = 0.
 * state  per tensor: step (applied steps), beta1_power = beta1^step and beta2_power = beta2^step as running products in float64 (1
 *        before the first step), and the two float32 factors of the update, step_size = lr / (1 - beta1_power) and inv_sqrt_bc2 =
 *        1 / sqrt(1 - beta2_power), both computed in float64 and rounded once.
 * global applied / skipped steps since the caller zeroed them; of the last call: nonfinite (gradient elements that are NaN or +-Inf),
 *        sumsq (of the finite ones), clip = float32(min(1, max_norm / (sqrt(sumsq) + 1e-6))) (1 for max_norm <= 0: no limit), apply =
 *        (nonfinite == 0), watch_nonfinite.
 *
 * lav_optim_adam_step: three launches on `stream` (statistics per chunk; one workgroup that reduces them in a fixed order, decides and
 * advances the words of every tensor of the table; the update per chunk).  With apply set, in float32, every operation rounded on its own
 * (beta, 1 - beta and eps are the row's float64 values rounded once):
 *     g' = g * clip;  m = beta1 m + (1 - beta1) g';  v = beta2 v + ((1 - beta2) g') g';  p = p - step_size (m / (sqrt(v) inv_sqrt_bc2 + eps))
 * Without it nothing is stored but `skipped` + 1 and the statistics words: p, m, v and the tensors' words keep every bit.
 * lav_optim_grad_stats: the first two launches, writing the five statistics words of `global` only.
 * No host synchronisation, no float atomic, no dependency between workgroups of one launch; identical inputs give identical bits.
 * workspace: DEVICE, 256-byte aligned, lav_optim_workspace_bytes(total_chunks, watch_chunks) bytes (0 for counts the calls would
 * refuse); needs no initialisation.
 */
typedef struct lav_optim_tensor {
    float *p;
    const float *g;
    float *m;
    float *v;
    long long numel;
    double lr, beta1, beta2, eps;
    int state;
    int chunk0;
} lav_optim_tensor;

typedef struct lav_optim_watch {
    const float *data;
    long long numel;
    int chunk0;
    int reserved;
} lav_optim_watch;

typedef struct lav_optim_state {
    long long step;
    double beta1_power, beta2_power;
    float step_size, inv_sqrt_bc2;
} lav_optim_state;

typedef struct lav_optim_global {
    long long applied, skipped, nonfinite;
    double sumsq;
    float clip;
    int apply;
    long long watch_nonfinite;
} lav_optim_global;

int lav_optim_chunk(void);
size_t lav_optim_workspace_bytes(long long total_chunks, long long watch_chunks);
int lav_optim_grad_stats(const lav_optim_tensor *table, int ntensors, int total_chunks, const lav_optim_watch *watch, int nwatch,
                         int watch_chunks, lav_optim_global *global, double max_norm, void *workspace, size_t workspace_bytes, void *stream);
int lav_optim_adam_step(const lav_optim_tensor *table, int ntensors, int total_chunks, const lav_optim_watch *watch, int nwatch,
                        int watch_chunks, lav_optim_state *state, lav_optim_global *global, double max_norm, void *workspace,
                        size_t workspace_bytes, void *stream);

/* lav_optim_adam_ema_step (ABI 48; FusedAdam(ema_decay=...), the trainers' --ema): lav_optim_adam_step, and the update launch also keeps
 * an exponential moving average of every tensor of the table.  shadow: a DEVICE array of ntensors float pointers, row-parallel to `table`
 * (shadow[r] belongs to table[r]): float32, dense, numel elements, 4-byte aligned, overlapping none of p, g, m, v.  ema_decay: 0 < decay < 1,
 * anything else is refused.  With the tensor's words advanced to the step count k >= 1, once per workgroup in float64
 *     d_k = min(ema_decay, (1 + k) / (10 + k));  omd = float32(1 - d_k)
 * and per element in float32, every operation rounded on its own, with p the parameter the launch has just computed:
 *     e = e + omd (p - e)
 * With apply clear e keeps every bit, as p, m and v do.  Same three launches, same workspace, same structs; p, m, v, the words and `global`
 * get the bits lav_optim_adam_step gives them.  16-byte accesses where p, m, v and e share a misalignment, 4-byte accesses otherwise.
 * Specification: lav_amd.train.optim.fused_adam_numpy(..., ema_decay=), equal in every stored bit. */
int lav_optim_adam_ema_step(const lav_optim_tensor *table, int ntensors, int total_chunks, const lav_optim_watch *watch, int nwatch,
                            int watch_chunks, lav_optim_state *state, lav_optim_global *global, double max_norm, float *const *shadow,
                            double ema_decay, void *workspace, size_t workspace_bytes, void *stream);

/* lav_optim_tensor_stats (ABI 50; FusedAdam.tensor_stats(), the trainers' --tensor-stats N): the per-tensor view of a step, over the
 * step's own table, watch rows and state words.  It reads g, p, m, v of every tensor once and stores nothing into them, into `state` or
 * into any global word.  rows_out [ntensors] and watch_out [nwatch] in DEVICE memory, 8-byte aligned, row-parallel to the tables:
 *   gradient g   g_nonfinite (NaN, +-Inf), g_zeros (+-0), g_sumsq (float64, of the finite elements), g_maxabs (the largest finite |g|),
 *                hist[64]: a finite element with biased exponent field e counts in bin clamp(e - 86, 0, 63) - bin 0: zeros, denormals and
 *                everything below 2^-40; bin k (1 .. 62): [2^(k-41), 2^(k-40)); bin 63: finite values >= 2^22.  Elements that are not
 *                finite count in g_nonfinite alone.
 *   parameter p  p_nonfinite, p_sumsq, p_maxabs, as for g.
 *   update u     u_sumsq, u_maxabs over the finite elements of u = step_size * (m / (sqrtf(v) * inv_sqrt_bc2 + eps)) in float32, every
 *                operation rounded on its own, from the tensor's state words and m, v as they stand: after an applied step the value the
 *                update launch subtracted, in every bit; after a skipped one the previous applied update.  A tensor at step 0 gives 0.
 *   watched      nonfinite, maxabs.
 * Integers, bins and the bit patterns of the maxima are exact; a sum of squares is within numel * 2^-53 relative of any other order.
 * Two launches on `stream`: a workgroup per chunk leaves its partials (per-chunk bins are 16-bit) in the workspace, then a wave per
 * tensor reduces them in chunk order.  No float atomic, no dependency between workgroups of one launch: identical inputs give identical
 * bits.  workspace: DEVICE, 256-byte aligned, lav_optim_tensor_stats_workspace_bytes(total_chunks, watch_chunks) bytes (0 for counts the
 * call would refuse); needs no initialisation.  Specification: lav_amd.train.optim.tensor_stats_numpy.
 *
 * lav_optim_blame (ABI 50): who caused a skipped step.  One workgroup behind a lav_optim_adam_step / lav_optim_adam_ema_step on the same
 * stream, with the same tables, `global` and workspace: it reads the per-chunk counts that step left in the workspace, the tables and
 * `global`.  With global->apply == 0 one thread appends, in table order, the first (at most) LAV_OPTIM_BLAME_PER_STEP tensors whose
 * gradient holds elements that are not finite to ring[0], and the first (at most) as many watched buffers with such elements to ring[1]:
 * record k of a ring (counted from 0 since the caller zeroed the block) lies in slot k % LAV_OPTIM_BLAME_RING, written[] counts the
 * records ever appended.  A record: step = applied + skipped (the ordinal of the skipped step), index = the row's `state` (for a
 * buffer: its row in `watch`), nonfinite = its count.  With apply == 1 nothing is written.
 * Specification: lav_amd.train.optim.blame_numpy. */
#define LAV_OPTIM_HIST_BINS 64
#define LAV_OPTIM_BLAME_RING 16
#define LAV_OPTIM_BLAME_PER_STEP 4

typedef struct lav_optim_tensor_row {
    double g_sumsq, p_sumsq, u_sumsq;
    long long g_nonfinite, g_zeros, p_nonfinite;
    float g_maxabs, p_maxabs, u_maxabs;
    int reserved;
    long long hist[LAV_OPTIM_HIST_BINS];
} lav_optim_tensor_row;

typedef struct lav_optim_watch_row {
    long long nonfinite;
    float maxabs;
    int reserved;
} lav_optim_watch_row;

typedef struct lav_optim_blame_record {
    long long step, nonfinite;
    int index;
    int reserved;
} lav_optim_blame_record;

typedef struct lav_optim_blame_block {
    long long written[2];                                       /* [0] tensors, [1] watched buffers */
    lav_optim_blame_record ring[2][LAV_OPTIM_BLAME_RING];
} lav_optim_blame_block;

size_t lav_optim_tensor_stats_workspace_bytes(long long total_chunks, long long watch_chunks);
int lav_optim_tensor_stats(const lav_optim_tensor *table, int ntensors, int total_chunks, const lav_optim_watch *watch, int nwatch,
                           int watch_chunks, const lav_optim_state *state, lav_optim_tensor_row *rows_out, lav_optim_watch_row *watch_out,
                           void *workspace, size_t workspace_bytes, void *stream);
int lav_optim_blame(const lav_optim_tensor *table, int ntensors, int total_chunks, const lav_optim_watch *watch, int nwatch,
                    int watch_chunks, const lav_optim_global *global, lav_optim_blame_block *blame, const void *workspace,
                    size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * lav_eval_resample (ABI 49; the eval tools' --bootstrap, lav_amd.ops.eval_resample): block-bootstrap replicates of a table of
 * accumulator rows.  rows [R][W] int64 in DEVICE memory, one row per block of consecutive frames (EvaluatorBase.resample); out
 * [B + 1][W] int64 in DEVICE memory, overlapping no row; both 8-byte aligned.
 *     out[0][w] = sum over r of rows[r][w]                       the identity replicate: no draws, the run's own accumulator
 *     out[b][w] = sum over j < R of rows[idx(b, j)][w]           b = 1 .. B
 *     idx(b, j) = (u * R) >> 32 as a 64-bit product, u = word j & 3 of Philox4x32-10 at counter (j >> 2, b, 0x52534D50, 0) and key
 *                 (seed & 0xffffffff, seed >> 32) - lav_augment_u8's generator
 * The multiply-high map favours some rows by at most R / 2^32 (below 2.5e-4 at the cap).  Sums are int64 sums modulo 2^64: any
 * split of the work gives the same bits.  1 <= R <= 2^20, W >= 1, B >= 0, R W 8 <= 4 GiB; anything else is refused before the launch.
 * One launch on `stream`: a workgroup per replicate and tile of up to 64 columns, which draws the replicate's indices into LDS
 * lav_eval_resample_chunk() at a time; no atomics, no floating point, no dependency between workgroups, nothing copied to the host.
 * Specification: lav_amd.train.eval_common.eval_resample_numpy, equal in every word. */
int lav_eval_resample_chunk(void);
int lav_eval_resample(const long long *rows, int R, int W, int B, unsigned long long seed, long long *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LAV_AMD_H */
