/*
 * mvs_amd.h -- C-ABI of the MI355X-native MVS patch-expansion library
 * (libmvs_amd.so, built from
 *  simple-implementation-of-structure-from-motion-and-multi-view-stereo-by-python_amd/csrc).
 *
 * The reference (MarvinChung/simple-implementation-of-structure-from-motion-
 * and-multi-view-stereo-by-python) is pure Python with no FFI; each entry point
 * below names the Python interface it replaces.  Conventions:
 *   - plain pointers and sizes, no torch / C++ types;
 *   - every call returns 0 on success or a negative status
 *     (MVS_E_ARG, MVS_E_HIP, MVS_E_UNSUPPORTED, MVS_E_NOMEM); the message is in
 *     mvs_last_error(ctx) (or mvs_last_error(NULL) when create failed);
 *   - no C++ exception crosses the ABI;
 *   - one context per device, driven by one host thread; *_device calls are
 *     ordered on the caller's HIP stream (NULL = the context's stream).
 *
 * Arrays follow the reference's numpy conventions: K/R row-major 3x3 per view
 * (V*9 doubles), t 3 per view, images V*H*W*3 uint8 RGB (main.py:17-18), view
 * index = position in the sorted image list = par-file row - 1 (utils.py:72-80).
 */
#ifndef MVS_AMD_H
#define MVS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_OK 0
#define MVS_E_ARG (-1)
#define MVS_E_HIP (-2)
#define MVS_E_UNSUPPORTED (-3)
#define MVS_E_NOMEM (-4)
#define MVS_E_DIVZERO (-5)   /* the reference would raise ZeroDivisionError (filter_out_outlier) */

typedef struct mvs_ctx mvs_ctx;
typedef struct mvs_stage_result mvs_stage_result;
typedef struct mvs_stage mvs_stage;

/* Library version string. */
const char* mvs_version(void);

/* Scene setup: replaces the per-call work the reference redoes on every photo
 * test -- read_pars (utils.py:56-81, called at MVS2.py:178/309), the per-call
 * full-frame copy + cvtColor(BGR2GRAY) (HarrisFeatures.py:124-125) and
 * cv2.Rodrigues(par_r) (utils.py:242).  Uploads the images once, builds the
 * device gray stack (OpenCV BGR2GRAY fixed-point formula applied to the RGB
 * data, as the reference does) and the per-view camera table.
 * Rp may be NULL (the library computes R' = Rodrigues(Rodrigues(R))).
 * 1 <= V <= 256, 16 <= H, W <= 65536. */
int mvs_ctx_create(int device, int V, int H, int W, const uint8_t* rgb, const double* K,
                   const double* R, const double* t, const double* Rp, mvs_ctx** out);
void mvs_ctx_destroy(mvs_ctx* ctx);
const char* mvs_last_error(const mvs_ctx* ctx);
/* Copies the rotations the projection uses (V*9) -- for parity tests. */
int mvs_ctx_rproj(const mvs_ctx* ctx, double* Rp);
/* The device part of the scene setup again, from the resident RGB images:
 * the gray stack and its signed view-major copy (k_build_scene), and the
 * window-moment tables built so far (k_moments).  For measuring a cold sweep
 * (setup + scoring) and after mvs_ctx_set_images; stream-ordered (NULL = the
 * context's stream). */
int mvs_ctx_rebuild(mvs_ctx* ctx, void* stream);
/* Replaces the resident RGB images of views [first_view, first_view + n_views)
 * by rgb (n_views*H*W*3 uint8, host), on the device and in the host copy the
 * stage's colours come from.  Synchronous on the context's stream; no call of
 * the context may be in flight on another stream.  The gray stack, its
 * view-major copy and the window-moment tables still hold the old images
 * until mvs_ctx_rebuild. */
int mvs_ctx_set_images(mvs_ctx* ctx, int first_view, int n_views, const uint8_t* rgb);

/* Batched MyPatch.photo_consistenecy_test (MVS2.py:62-77): for candidate i
 * with centre c[3i..3i+2] and reference view ref[i], project into ref[i]
 * (projectPoint, utils.py:241-244), take the (2*wid+1)^2 windows of every view
 * at that pixel (getDescFeatures, HarrisFeatures.py:116-133; all views at the
 * reference view's pixel, MVS2.py:68), and keep the views idx != ref with
 * ctNcc > min_ncc (MVS2.py:39-43, 72).
 * Outputs: xy[2i..] = projection (the x, y of every V entry, MVS2.py:74);
 * mask[i*words + w] bit b = view 64w+b passed (words = ceil(V/64));
 * count[i] = |V|; avg[i] = mean ncc of the passing views (avg_ncc_score).
 * Host pointers; synchronous. wid in 1..5. */
int mvs_score(mvs_ctx* ctx, int64_t n, const double* c, const int32_t* ref, int wid,
              double min_ncc, double* xy, uint64_t* mask, int32_t* count, double* avg);
/* Same on device pointers (e.g. torch tensor data_ptr()), stream-ordered.
 * Calls on different streams are ordered too: a call waits for the previous
 * call's use of the context's scratch (an event on that call's stream).
 * d_avg may be NULL when avg_ncc_score is not needed (it only feeds the
 * disabled filter_out_outlier, MVS2.py:281).
 * Device memory: the first tiled call with a given wid builds that wid's
 * window-moment tables, kept for the context's life: (H*W + 16) * VP
 * entries (VP = V rounded up to 16, or to 64 at V > 64) of 10 B at
 * V <= 64 (S_b int16 + w binary64) or 6 B at V > 64 (S_b int16 + D int32)
 * -- 147 MB per wid for dinoRing (48 x 640 x 480), 3.2 GB for
 * 256 x 1920 x 1080.  Past 2^31
 * entries, or when the allocation fails, that scene is scored with the
 * in-kernel moments instead (same results, slower). */
int mvs_score_device(mvs_ctx* ctx, int64_t n, const double* d_c, const int32_t* d_ref, int wid,
                     double min_ncc, double* d_xy, uint64_t* d_mask, int32_t* d_count,
                     double* d_avg, void* stream);
/* The same photo test with one record per candidate instead of three arrays:
 * d_rec[i * (words + 1) ...] = [mask words of i, avg_ncc_score as binary64
 * bits]; |V| = the popcount of the mask words.  One 16-B store per candidate
 * at V <= 64 (the scorer's output stores are scattered by candidate id).
 * d_rec 16-B aligned; mvs_pack_accepted reads it with d_count = NULL. */
int mvs_score_device_rec(mvs_ctx* ctx, int64_t n, const double* d_c, const int32_t* d_ref, int wid,
                         double min_ncc, double* d_xy, int64_t* d_rec, void* stream);
/* Plane-warped, per-view reprojected photo-consistency test (no reference
 * counterpart: photo_consistenecy_test cuts every view's window at the
 * reference view's pixel, MVS2.py:68, and never uses the patch normal).
 * Candidate i: centre c[3i..], unit normal nrm[3i..] pointing towards the
 * cameras (NOT checked or normalised), reference view r = ref[i].
 * Cameras: rotation = mvs_ctx_rproj's, translation t, fx fy cx cy (no skew),
 * O_v = -Rp_v^T t_v; integer coordinates are pixel centres; gray = the
 * context's gray stack.
 *   1. (x, y) = projection of c into r -> xy (bit-equal to mvs_score's).
 *   2. The candidate is invalid (count 0, empty mask, avg 0, every ncc nan)
 *      unless depth in r > 0, x >= 0, y >= 0, the window
 *      [x0-wid, x0+wid] x [y0-wid, y0+wid] around (x0, y0) = (int(x), int(y))
 *      lies inside [0, W-1] x [0, H-1], nrm.(O_r - c) > min_cos |O_r - c|,
 *      and the reference window a is not constant (N sum a^2 - (sum a)^2 > 0,
 *      N = (2 wid + 1)^2).
 *   3. Every window pixel q goes to the patch plane: d = Rp_r^T ((q.x-cx_r)/
 *      fx_r, (q.y-cy_r)/fy_r, 1), X = O_r + d (nrm.(c-O_r)) / (nrm.d).
 *   4. A view v != r is tested when nrm.(O_v - c) > min_cos |O_v - c|.  It
 *      fails (ncc nan, bit clear) unless every X has depth > 0 in v, every
 *      sample position (sx, sy) = projection of X into v has 0 <= sx <= W-1,
 *      0 <= sy <= H-1, and the warped window b is not constant.
 *   5. b = bilinear sample in difference form: ix = floor(sx), ax = sx - ix,
 *      ix1 = min(ix+1, W-1) (same in y); top = g00 + ax (g01 - g00), bot =
 *      g10 + ax (g11 - g10), b = top + ay (bot - top) -- exact on a constant
 *      neighbourhood, so a flat warped window has D_b = 0 and fails.
 *   6. ncc = (N sum ab - sum a sum b) / sqrt(D_a D_b) * N/(N-1) (ctNcc's
 *      scaling, MVS2.py:39-43); the view passes when ncc > min_ncc.
 * Positions, samples and sums are binary64; results are deterministic.
 * Outputs as mvs_score: xy (n*2), mask (n*words), count, avg = mean ncc of
 * the passing views; ncc[i*V + v] (binary64; nan for r, culled and failed
 * views).  avg and ncc may be NULL.  wid in 1..5, min_cos in [0, 1).
 * n = 0 returns MVS_OK, launches nothing and touches no context state;
 * MVS_E_ARG (message in mvs_last_error) for wid or min_cos out of range, a
 * NULL required pointer, n < 0 and (host call) a ref outside 0..V-1.
 * The call uses none of the scorers' scratch or counter sets (one kernel,
 * k_score_warp, reading the scene only): it may be interleaved freely with
 * every other call.  Host pointers; synchronous. */
int mvs_score_warped(mvs_ctx* ctx, int64_t n, const double* c, const double* nrm, const int32_t* ref,
                     int wid, double min_ncc, double min_cos, double* xy, uint64_t* mask,
                     int32_t* count, double* avg, double* ncc);
/* Same on device pointers, stream-ordered (NULL = the context's stream); a
 * ref outside 0..V-1 makes its candidate invalid with xy = nan. */
int mvs_score_warped_device(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm,
                            const int32_t* d_ref, int wid, double min_ncc, double min_cos,
                            double* d_xy, uint64_t* d_mask, int32_t* d_count, double* d_avg,
                            double* d_ncc, void* stream);
/* One level of a fixed-grid depth and normal refinement of patches against
 * the plane-warped photo test (no reference counterpart: the reference never
 * refines a patch).  Cameras, gray values, pixel conventions and the bilinear
 * form are mvs_score_warped's.
 * Candidate i: centre c[3i..], unit normal nrm[3i..] towards the cameras (NOT
 * checked or normalised), reference view r = ref[i], a view list
 * views[i*tv .. i*tv+tv-1] (tv in 1..32, unused slots -1 at the end; |T| = the
 * number of entries >= 0) and a depth step dstep[i] > 0 in world units.
 * Scalars: wid in 1..5, min_cos in [0, 1), kd in 0..3, ka in 0..2, astep >= 0
 * in radians, step_scale > 0, ka astep step_scale <= 1.2.
 *   1. Window.  (x, y) = mvs_score_warped's projection of c into r, (x0, y0) =
 *      (int(x), int(y)).  The candidate must pass step 2 of mvs_score_warped
 *      with c and nrm, |T| >= 1 and dstep > 0.  The window and its values a
 *      are the same for every hypothesis (c_k below lies on the ray of c, so
 *      nothing is projected again).
 *   2. Grid.  u = (c - O_r) / |c - O_r|, c_k = c + (k dstep step_scale) u for
 *      k = -kd..kd.  m = the index of the smallest |nrm_m| (lowest index on
 *      ties), e1 = (nrm x axis_m) / |nrm x axis_m|, e2 = nrm x e1,
 *      n_ij = (nrm + tan(i alpha) e1 + tan(j alpha) e2) / |...| with alpha =
 *      astep step_scale for i, j = -ka..ka; n_00 = nrm as given.  The 2 ka + 1
 *      tangents are computed once on the host (libm tan).  Hypothesis
 *      h = ((k + kd) A + (j + ka)) A + (i + ka), A = 2 ka + 1,
 *      H = (2 kd + 1) A^2; the centre hypothesis (H - 1) / 2 is the input.
 *   3. Score.  Hypothesis h is the plane through c_k with normal n_ij; every
 *      window pixel's ray meets it as in step 3 of mvs_score_warped.  It is
 *      valid only when n_ij.(O_r - c_k) > min_cos |O_r - c_k| and every list
 *      view passes the facing test of step 4 with (n_ij, c_k) and gets a
 *      finite ncc from steps 4-6.  score[h] = (sum of the list's ncc, in list
 *      order) / |T|, nan when invalid.  There is no min_ncc: the list is the
 *      caller's choice of views.
 *   4. Choice.  The centre hypothesis is kept unless another valid one scores
 *      strictly higher; among the others the highest score wins, ties go to
 *      the lowest index.  best[i] = the chosen index, score_best[i] = its
 *      score (the same bits as scores[i*H + best]), c_out / nrm_out = its c_k
 *      and n_ij -- for the centre the inputs, bit for bit.  With no valid
 *      hypothesis or an invalid candidate: best = -1, score_best = nan,
 *      c_out / nrm_out = the inputs bit for bit, every scores entry nan.
 * scores (n*H) may be NULL.  c_out / nrm_out must not overlap c / nrm.
 * Binary64 throughout; results are deterministic.  n = 0 returns MVS_OK and
 * launches nothing.  MVS_E_ARG (message in mvs_last_error) for a scalar out of
 * range, a NULL required pointer, n < 0 and (host call) a ref outside 0..V-1
 * or a list entry outside -1..V-1, equal to r, repeated, or following a -1.
 * The call uses none of the scorers' scratch or counter sets (one kernel,
 * k_refine_warp, reading the scene only): it may be interleaved freely with
 * every other call.  Host pointers; synchronous. */
int mvs_refine_warped(mvs_ctx* ctx, int64_t n, const double* c, const double* nrm, const int32_t* ref,
                      const int32_t* views, int tv, const double* dstep, int wid, double min_cos, int kd,
                      int ka, double astep, double step_scale, double* c_out, double* nrm_out,
                      int32_t* best, double* score_best, double* scores);
/* Same on device pointers, stream-ordered (NULL = the context's stream); a
 * ref outside 0..V-1 or a list that breaks the rules above makes its
 * candidate invalid. */
int mvs_refine_warped_device(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm,
                             const int32_t* d_ref, const int32_t* d_views, int tv, const double* d_dstep,
                             int wid, double min_cos, int kd, int ka, double astep, double step_scale,
                             double* d_c_out, double* d_nrm_out, int32_t* d_best, double* d_score_best,
                             double* d_scores, void* stream);
/* What mvs_refine_warped is fed, built from mvs_score_warped's per-view ncc
 * (no reference counterpart): per output row k a view list and a depth step.
 * The source row is s = sel ? sel[k] : k, a row of ncc (rows x V), c (rows x 3)
 * and ref (rows); views is n x max_views, dstep is n.
 *   View list, from ncc[s*V .. s*V+V-1]:
 *   1. view v passes when ncc_v > min_ncc (a binary64 comparison: nan never
 *      passes, +inf does);
 *   2. a passing view v is selected when fewer than max_views passing views u
 *      have ncc_u > ncc_v, or ncc_u == ncc_v with u < v (numeric comparison:
 *      -0.0 equals +0.0) -- the max_views best, ties to the lower view;
 *   3. the selected views go to views[k*max_views ..] in ascending view order,
 *      the remaining slots are -1.
 *   The list does not depend on ref (the scorer leaves ncc of r at nan).
 *   Depth step, with r = ref[s], c = c[3s..]: depth = Rp_r[2][0] c.x +
 *   Rp_r[2][1] c.y + Rp_r[2][2] c.z + t_r[2] (products and sums left to right,
 *   unfused), dstep[k] = (depth_px depth) / ((fx_r + fy_r) / 2): the world size
 *   of depth_px pixels at the patch (not clamped: <= 0 or nan for a centre on or
 *   behind the camera plane or a nan centre, which mvs_refine_warped rejects).
 * MvsContext.refine_view_lists and refine_depth_steps restate both in numpy;
 * the results are equal bit for bit.
 * sel may be NULL (then n <= rows).  dstep may be NULL: lists only, c and ref
 * are then not read and may be NULL.  max_views in 1..32, min_ncc not nan,
 * depth_px finite and > 0.  n = 0 returns MVS_OK and launches nothing.
 * MVS_E_ARG (message in mvs_last_error) for a scalar out of range, n < 0,
 * rows < 0, n > rows without sel, a NULL required pointer and (host call) a
 * sel entry outside 0..rows-1 or a ref outside 0..V-1.
 * Device pointers, stream-ordered (NULL = the context's stream).  A sel entry
 * outside 0..rows-1 gives an all -1 list and dstep nan and reads nothing of
 * that row; a ref outside 0..V-1 gives dstep nan.
 * One kernel (k_refine_lists: one wave per row, lane = view) that reads the
 * camera table and its arguments only: no scratch, no atomics, no counter sets
 * and no context state.  It may be interleaved freely with every other call and
 * run on several streams at once. */
int mvs_refine_lists_device(mvs_ctx* ctx, int64_t n, int64_t rows, const int64_t* d_sel,
                            const double* d_ncc, const double* d_c, const int32_t* d_ref,
                            double min_ncc, int max_views, double depth_px, int32_t* d_views,
                            double* d_dstep, void* stream);
/* Same on host pointers; synchronous, on the context's stream and its own
 * staging buffers. */
int mvs_refine_lists(mvs_ctx* ctx, int64_t n, int64_t rows, const int64_t* sel, const double* ncc,
                     const double* c, const int32_t* ref, double min_ncc, int max_views,
                     double depth_px, int32_t* views, double* dstep);
/* ---- Level-synchronous patch expansion driven by the plane-warped test ----
 * (no reference counterpart: patch_expansion, MVS2.py:308-404, ignores the
 * normal, cuts every view's window at the reference view's pixel and never
 * refines).  Three stream-ordered device primitives that a caller runs between
 * mvs_score_warped_device and mvs_refine_warped_device calls; the chain is
 * MvsContext.expand_warped.  Cameras (Rp, t, fx fy cx cy, O_v = -Rp_v^T t_v) are
 * mvs_score_warped's; "projection" is mvs_score's, (x, y, depth).
 * Cell grid of cell_size s in 1..16: nci = W / s, ncj = H / s (integer
 * division; pixels past the last full cell belong to no cell); the cell of a
 * pixel position (x, y) is (int(x) / s, int(y) / s); the centre of cell (i, j)
 * is the pixel position (i s + (s-1)/2, j s + (s-1)/2).  Occupancy is
 * occ[v][j][i], uint8, caller-owned, V ncj nci bytes, nonzero = taken.
 * A job is four int32 (p, v, i, j); job arrays are 16-B aligned.
 *
 * mvs_wexp_children_device: child jobs and geometry of n frontier patches
 * (centre c[3p..], normal nrm[3p..], reference view ref[p], mask[p*words..]).
 * Per patch p:
 *   1. the views {ref_p} U {v : mask bit v} (those in 0..V-1) in ascending order;
 *   2. (x, y, depth) = projection of c_p into v; v is skipped unless depth > 0,
 *      0 <= x < W, 0 <= y < H (which leaves out nan and inf) and the cell (i, j)
 *      of (x, y) lies inside the grid;
 *   3. the neighbours k = 0..3: (i+1, j), (i-1, j), (i, j+1), (i, j-1); one
 *      outside the grid or with occ[v][j'][i'] != 0 is skipped;
 *   4. q = that cell's centre, d = Rp_v^T ((q.x-cx_v)/fx_v, (q.y-cy_v)/fy_v, 1),
 *      den = nrm_p.d, s = nrm_p.(c_p - O_v) / den; skipped unless den != 0 and s
 *      is finite and > 0;
 *   5. X = O_v + s d; skipped unless |X - c_p| <= max_dist (> 0, world units);
 *   6. the child: centre X, the parent's normal bit for bit, reference view v,
 *      job (p, v, i', j').
 * d_total[0] = the number of jobs found (it may exceed cap >= 0).  The jobs are
 * compacted in exactly that sequential order (p, then view, then k) into
 * d_job (cap*4), d_cc, d_cn (cap*3) and d_cref (cap); only the first cap are
 * written (cap = 0 counts only: the four arrays may then be NULL).  Two parents may name the same (v, cell): both are kept, the claim
 * decides.  Products and sums are taken left to right in binary64, unfused; the
 * order across patches comes from a count pass, a scan and an emit pass
 * (k_wexp_children, k_wexp_scan), never from atomics: results are deterministic.
 *
 * mvs_wexp_claim_device: one winner per (view, cell) among m jobs.  A job
 * contends when accept != 0 and its score is finite; among the contenders of
 * one (v, i, j) the highest score wins, compared numerically (-0.0 = +0.0),
 * ties to the lowest job index.  d_win[k] = 1 for winners, 0 for every other
 * job.  A job whose (v, i, j) lies outside 0..V-1 x nci x ncj never wins; the
 * host-pointer variant mvs_wexp_claim (synchronous) returns MVS_E_ARG for it.
 * The context keeps a per-(view, cell) grid of 12 B per cell, allocated at the
 * first call and left zero by every call: only the cells that the jobs name
 * are touched (k_wexp_claim_max / _min / _win / _reset: 64-bit atomic max of an
 * order-preserving image of the score, then of the complemented index among
 * its holders).  The result does not depend on scheduling.
 *
 * mvs_wexp_mark_device: for every job with d_win != 0, occ[cref][j][i] = 1 at
 * the job's own cell (no reprojection), and for every view v of the child's
 * final mask (d_mask, m*words) the cell of the projection of its centre
 * d_cc[3k..] into v, when depth > 0, 0 <= x < W, 0 <= y < H and the cell lies
 * inside the grid.  Other bytes stay as they are (k_wexp_mark).
 *
 * All three: n (m) = 0 returns MVS_OK, launches nothing and touches no context
 * state; MVS_E_ARG (message in mvs_last_error) for a scalar out of range, a
 * NULL pointer, n < 0 or a misaligned job array.  They use none of the scorers'
 * scratch or counter sets and may be interleaved freely with every other call;
 * calls on different streams are ordered on their own scratch. */
int mvs_wexp_children_device(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm,
                             const int32_t* d_ref, const uint64_t* d_mask, int cell_size,
                             const uint8_t* d_occ, double max_dist, int64_t cap, int32_t* d_job,
                             double* d_cc, double* d_cn, int32_t* d_cref, int64_t* d_total, void* stream);
int mvs_wexp_claim_device(mvs_ctx* ctx, int64_t m, const int32_t* d_job, const uint8_t* d_accept,
                          const double* d_score, int nci, int ncj, uint8_t* d_win, void* stream);
int mvs_wexp_claim(mvs_ctx* ctx, int64_t m, const int32_t* job, const uint8_t* accept, const double* score,
                   int nci, int ncj, uint8_t* win);
int mvs_wexp_mark_device(mvs_ctx* ctx, int64_t m, const int32_t* d_job, const uint8_t* d_win,
                         const double* d_cc, const int32_t* d_cref, const uint64_t* d_mask, int cell_size,
                         uint8_t* d_occ, void* stream);
/* ---- Visibility-consistency filter for warped patch sets ----
 * (no reference counterpart: filter_out_outlier below knows neither normals
 * nor depth order).  The fourth stage of the warped pipeline (test, refine,
 * expand, filter): it removes the patches that contradict the visibility of the
 * rest of the set.  Two stream-ordered device calls; the chain is
 * MvsContext.filter_warped.  Cameras, "projection" and the cell grid of
 * cell_size s in 1..16 are the expansion's above.
 *
 * Inputs: n patches, n < 2^31, with centre c[3p..], normal nrm[3p..], reference
 * view ref[p], mask[p*words..] and avg[p] (mvs_score_warped's), and the scalars
 * adj_px >= 0 (finite) and min_views >= 0.
 *   Views.  T(p) = {ref_p} U {v : mask bit v}, those in 0..V-1, ascending.  A row
 *   whose ref lies outside 0..V-1 is dead: it takes no part and gets vis 0,
 *   conf 0 and keep 0 (a chain drops patches by setting ref = -1, without
 *   compacting its arrays).
 *   Placement.  For v in T(p), (x, y, depth) = projection of c_p into v.  p is
 *   placed in v when depth > 0, 0 <= x < W, 0 <= y < H and the cell
 *   (int(x) / s, int(y) / s) lies inside the grid (mvs_wexp_mark's rule).  Its
 *   depth there is z_p(v) = Rp_v[6] X + Rp_v[7] Y + Rp_v[8] Z + t_v[2], products
 *   and sums left to right in binary64, unfused.
 *   Front grid.  front[v][j][i] (int32) = the placed patch of least z in that
 *   (view, cell), ties to the lowest index; zfront[v][j][i] (binary64) = its z.
 *   An empty cell holds -1 and +inf.  V ncj nci elements each.
 *   Adjacency of p and f in view v: d = c_p - c_f, a = |d.nrm_p| + |d.nrm_f|
 *   (each dot product left to right, unfused), rho = (adj_px z_p(v)) /
 *   ((fx_v + fy_v) / 2): adj_px pixel footprints at p's depth, the quantity of
 *   mvs_refine_lists' depth step.  Adjacent iff a < 2 rho; a nan anywhere makes
 *   them not adjacent.
 *   Visibility.  Bit v of vis(p) (n*words uint64) is set iff p is placed in v
 *   and front = p there or p is adjacent in v to the front patch there.
 *   Conflicts.  F(p) = the SET of front patches f over p's placed views with
 *   f != p and f not adjacent to p in that view: a patch named in several views
 *   counts once, and it belongs to F(p) as soon as one placed view has it in
 *   front and not adjacent (adjacency depends on the view through z_p(v)).
 *   Weights.  w(p) = floor(clamp(avg_p, 0, 2) 2^32 + 0.5) as int64, 0 when avg_p
 *   is not finite (the product with 2^32 is exact).
 *   conf(p) = sum of w(f) over f in F(p) + sum of w(q) over the q with p in
 *   F(q), in int64: the evidence of the patches that hide p plus that of the
 *   patches p hides.  Two patches that hide each other in different views
 *   (p in F(q) and q in F(p)) are counted in both sums, so each gets the
 *   other's weight twice.  Integer sums do not depend on the order in which the
 *   atomic adds arrive.
 *   Decision.  keep(p) = alive and popcount(vis(p)) >= min_views and
 *   |T(p)| w(p) >= conf(p): PMVS's visibility count, and the patch's own
 *   support against its conflicting patches' support.
 *
 * mvs_wfilt_front_device writes every element of d_front and d_zfront (the
 * caller's two grids are its only scratch; n = 0 still fills them with -1 and
 * +inf): k_wfilt_fill, then k_wfilt_front twice -- a 64-bit atomic min of the
 * depth's bit pattern (positive doubles order as unsigned integers), then an
 * unsigned 32-bit atomic min of the index among the holders of the minimum.
 * mvs_wfilt_test_device reads a front grid as given -- it need not come from the
 * same rows, and a front patch need not be alive; an entry outside -1..n-1 is
 * read as -1 and a placed view whose cell holds -1 is neither visible nor a
 * conflict -- zeroes d_conf and writes d_vis, d_conf and d_keep (uint8) of every
 * row: k_wfilt_conflict (one wave per patch, lane = view; F(p) is made a set
 * inside the wave; one 64-bit atomic add of w(p) per member onto conf[f] and
 * one of the members' weights onto conf[p]), then k_wfilt_decide.  n = 0
 * returns MVS_OK and launches nothing.
 * Neither call keeps context state: they may run on any stream beside any other
 * call, and interleave freely with every other call.  Results are deterministic.
 * The host-pointer variants mvs_wfilt_front and mvs_wfilt_test are synchronous,
 * on the context's stream and the staging buffer that every host-pointer call
 * of the context shares (none keeps anything there past its return);
 * mvs_wfilt_test returns MVS_E_ARG for a front entry outside -1..n-1.
 * MVS_E_ARG (message in mvs_last_error) for a scalar out of range (cell_size,
 * adj_px negative, nan or inf, min_views < 0), a NULL pointer, n < 0 or
 * n >= 2^31. */
int mvs_wfilt_front_device(mvs_ctx* ctx, int64_t n, const double* d_c, const int32_t* d_ref,
                           const uint64_t* d_mask, int cell_size, int32_t* d_front, double* d_zfront,
                           void* stream);
int mvs_wfilt_test_device(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm,
                          const int32_t* d_ref, const uint64_t* d_mask, const double* d_avg, int cell_size,
                          double adj_px, int min_views, const int32_t* d_front, uint64_t* d_vis,
                          int64_t* d_conf, uint8_t* d_keep, void* stream);
int mvs_wfilt_front(mvs_ctx* ctx, int64_t n, const double* c, const int32_t* ref, const uint64_t* mask,
                    int cell_size, int32_t* front, double* zfront);
int mvs_wfilt_test(mvs_ctx* ctx, int64_t n, const double* c, const double* nrm, const int32_t* ref,
                   const uint64_t* mask, const double* avg, int cell_size, double adj_px, int min_views,
                   const int32_t* front, uint64_t* vis, int64_t* conf, uint8_t* keep);
/* ---- Neighbour-support test for warped patch sets ----
 * PMVS's third filter on the front grid: a patch stays when enough of the
 * patches next to it, in the images it is seen in, lie on its surface.  One
 * stream-ordered device call (k_wfilt_support); MvsContext.filter_warped runs it
 * after the visibility passes when given min_support.  The patch set, T(p),
 * placement, the front grid and adjacency are the visibility filter's above,
 * unchanged; adj_px >= 0 (finite), min_support in [0, 1] (finite), min_neigh >= 0.
 *   Incidences.  For a live patch p and every v in T(p) in which p is placed,
 *   in cell (i, j): the eight cells (i + di, j + dj), di, dj in {-1, 0, 1}
 *   without (0, 0), that lie inside the grid (0 <= i + di < nci, 0 <= j + dj <
 *   ncj).  q = front[v][j + dj][i + di]; an entry outside -1..n-1 reads as -1.
 *   q = -1 and q = p are skipped.  The grid is taken as given: the centre and
 *   normal of a named row are read whether or not that row is alive, and the
 *   grid need not come from the same rows.
 *   N(p) (int32) = the number of the remaining incidences (v, di, dj).
 *   A(p) (int32) = the number of those in which p and q are adjacent in view v:
 *   d = c_p - c_q, |d.nrm_p| + |d.nrm_q| < 2 rho, rho = (adj_px z_p(v)) /
 *   ((fx_v + fy_v) / 2), each operation in the visibility filter's order,
 *   unfused; a nan anywhere makes them not adjacent.
 *   Incidences are counted, not distinct patches: a front patch that fills
 *   several neighbour cells, or the neighbour cells of several views, counts
 *   once per cell and view.  N and A are plain integer sums.
 *   Decision.  keep(p) = alive and N(p) >= min_neigh and (double)A(p) >=
 *   min_support * (double)N(p), the product one binary64 multiply.
 *   A dead row gets N = A = 0 and keep = 0.
 * Only the front patch of a neighbour cell counts, not every patch that
 * projects into it (PMVS's C(p) holds all of them).
 * mvs_wfilt_support_device writes d_nb, d_adj (int32) and d_keep (uint8) of every
 * row and nothing else; n = 0 returns MVS_OK and launches nothing.  One wave
 * per patch, lane = view in groups of 64; the wave's sums come from cross-lane
 * shuffles.  No atomics, no scratch and no context state: it may run on any
 * stream beside any other call.  Results are deterministic.
 * The host-pointer variant mvs_wfilt_support is synchronous, on the context's
 * stream and the host-pointer calls' shared staging buffer, and returns
 * MVS_E_ARG for a front entry outside -1..n-1.
 * MVS_E_ARG (message in mvs_last_error) for a scalar out of range (cell_size,
 * adj_px negative, nan or inf, min_support nan or outside [0, 1], min_neigh <
 * 0), a NULL pointer, n < 0 or n >= 2^31. */
int mvs_wfilt_support_device(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm,
                             const int32_t* d_ref, const uint64_t* d_mask, int cell_size, double adj_px,
                             double min_support, int min_neigh, const int32_t* d_front, int32_t* d_nb,
                             int32_t* d_adj, uint8_t* d_keep, void* stream);
int mvs_wfilt_support(mvs_ctx* ctx, int64_t n, const double* c, const double* nrm, const int32_t* ref,
                      const uint64_t* mask, int cell_size, double adj_px, double min_support, int min_neigh,
                      const int32_t* front, int32_t* nb, int32_t* adj, uint8_t* keep);
/* ---- Seeds of the warped pipeline from image features ----
 * (no reference counterpart: the reference seeds from SfM tracks,
 * MVS2.py:196-262).  PMVS's match step: every feature of a view is paired with
 * the features of a neighbour view that lie along its epipolar line, and every
 * such pair is triangulated into an oriented seed candidate; the photo test
 * (mvs_score_warped) then tells the right candidates from the wrong ones and
 * round 0 of MvsContext.expand_warped keeps the best per (view, cell).  The chain
 * is MvsContext.seed_warped.  Cameras (Rp, t, fx fy cx cy, O_v = -Rp_v^T t_v)
 * are mvs_score_warped's; "projection" is mvs_score's, (x, y, depth); integer
 * coordinates are pixel centres; everything is binary64, unfused, products and
 * sums taken left to right.
 *
 * Inputs: the features of all views in one device array d_feat (F x 2 int32,
 * [col, row], mvs_harris_points' layout); feat_off (host, int64[V + 1],
 * feat_off[0] = 0, not decreasing, F = feat_off[V] < 2^31): the features of view
 * v are the rows feat_off[v] .. feat_off[v + 1] - 1; pairs (host, np x 2 int32):
 * ordered view pairs (r, v), r != v, both in 0..V-1 (a pair may repeat); epi_px
 * finite and > 0, min_sin2 in [0, 1), cap >= 0.
 * For pair k = (r, v), feature a of r at pixel q_a and feature b of v at q_b (a
 * and b local to their views):
 *   1. d_a = Rp_r^T ((q_a.x-cx_r)/fx_r, (q_a.y-cy_r)/fy_r, 1), d_b likewise in v,
 *      w = O_r - O_v.
 *   2. A = d_a.d_a, B = d_a.d_b, C = d_b.d_b, D = d_a.w, E = d_b.w, den = A C - B B.
 *      Skipped unless den > min_sin2 (A C): parallel rays and nan.
 *   3. s = (B E - C D) / den, u = (A E - B D) / den, the parameters of the two
 *      rays' closest points.  Skipped unless both are finite and > 0.
 *   4. X = O_r + s d_a: on a's ray, so the seed projects onto its own feature in r.
 *   5. (x, y, z) = projection of X into v.  Skipped unless z > 0 and err =
 *      (x - q_b.x)^2 + (y - q_b.y)^2 <= epi_px^2 (one binary64 product).
 *   6. The candidate: centre X, normal (O_r - X) / |O_r - X| (one sqrt, three
 *      divides), reference view r, cand row (k, a, b, v), err.
 * d_total[0] = the number of candidates (it may exceed cap).  They are compacted
 * in the order (pair k, then a, then b) into d_c, d_nrm (cap*3), d_ref (cap),
 * d_cand (cap*4 int32) and d_err (cap); only the first cap are written (cap = 0
 * counts only: the five arrays may then be NULL).  The order comes from a count
 * pass, a scan and an emit pass that repeats the count pass's arithmetic
 * (k_wseed_pairs, k_wseed_scan), never from atomics: two runs are bit-identical.
 * np = 0 or F = 0 returns MVS_OK, launches nothing and touches no context state
 * (d_total is then not written).  MVS_E_ARG (message in mvs_last_error) for
 * r = v, a view out of range, a feat_off that decreases or does not start at 0,
 * a scalar out of range, np < 0, a NULL required pointer, and pairs whose
 * reference views' features sum to 2^31 or more.
 * The call uses none of the scorers' scratch or counter sets and may be
 * interleaved freely with every other call; its per-row counts and offsets are
 * the expansion's scratch, and calls on different streams are ordered on it.
 * The host arrays are read before the call returns.  Stream-ordered (NULL = the
 * context's stream). */
int mvs_wseed_match_device(mvs_ctx* ctx, const int32_t* d_feat, const int64_t* feat_off, int64_t np,
                           const int32_t* pairs, double epi_px, double min_sin2, int64_t cap, double* d_c,
                           double* d_nrm, int32_t* d_ref, int32_t* d_cand, double* d_err, int64_t* d_total,
                           void* stream);
/* Same on host pointers; synchronous, on the context's stream and the
 * host-pointer calls' shared staging buffer. */
int mvs_wseed_match(mvs_ctx* ctx, const int32_t* feat, const int64_t* feat_off, int64_t np,
                    const int32_t* pairs, double epi_px, double min_sin2, int64_t cap, double* c, double* nrm,
                    int32_t* ref, int32_t* cand, double* err, int64_t* total);
/* The colour of n patches from the context's resident RGB images (k_wpatch_color:
 * one wave per patch, lane = view in groups of 64).  For patch p (centre
 * c[3p..], reference view ref[p], mask[p*words..]) and every view v of {ref_p} U
 * {v : mask bit v} inside 0..V-1 (a ref outside 0..V-1 names no view):
 *   1. (x, y, depth) = projection of c_p into v (mvs_score's);
 *   2. v counts when depth > 0, 0 <= x <= W-1 and 0 <= y <= H-1;
 *   3. per channel, S = the bilinear sample at (x, y) in mvs_score_warped's
 *      difference form (step 5 there) on the channel's bytes 0..255, unfused:
 *      top = g00 + ax (g01 - g00), bot = g10 + ax (g11 - g10), S = top + ay (bot - top);
 *   4. K = (int64) floor(S 256 + 0.5);
 *   5. color[3p + ch] = (double)(sum of K over the m counted views) / (double)(256 m):
 *      integer sums, so the result does not depend on the reduction order;
 *   6. m = 0 gives 0, 0, 0.
 * color (n*3 binary64), nviews (n int32) = m.  n = 0 returns MVS_OK and launches
 * nothing; MVS_E_ARG for n < 0, n >= 2^31 or a NULL pointer.  No scratch, no
 * atomics and no context state: it may run on any stream beside any other
 * call.  Stream-ordered (NULL = the context's stream). */
int mvs_wpatch_color_device(mvs_ctx* ctx, int64_t n, const double* d_c, const int32_t* d_ref,
                            const uint64_t* d_mask, double* d_color, int32_t* d_nviews, void* stream);
/* Same on host pointers; synchronous. */
int mvs_wpatch_color(mvs_ctx* ctx, int64_t n, const double* c, const int32_t* ref, const uint64_t* mask,
                     double* color, int32_t* nviews);
/* ---- Depth maps of a warped patch set ----
 * (no reference counterpart).  The far end of the warped pipeline: per-pixel
 * depth and patch-index maps of the views, rendered from the oriented patches
 * by a z-buffer splat; the count of the other views that agree with, or see
 * through, every pixel's depth; and the world points and colours of listed
 * pixels.  Three stream-ordered device calls; the chain that fuses the maps
 * into a dense cloud is MvsContext.depth_maps.  Cameras (Rp, t, fx fy cx cy,
 * O_v = -Rp_v^T t_v), "projection" (x, y, depth as mvs_score gives them), T(p)
 * = {ref_p} U {v : mask bit v} and the dead rows (ref outside 0..V-1) are the
 * visibility filter's above, word for word; mask bits >= V are ignored.
 * Integer coordinates are pixel centres.  All arithmetic is binary64, products
 * and sums left to right, unfused, so every output is defined to the bit.
 * Maps cover a contiguous view range v0 .. v0 + nv - 1 inside 0..V-1 (nv >= 1),
 * are laid out [v - v0][y][x] (nv H W elements) and belong to the caller; no
 * call keeps context state, so each runs on any stream beside any other call.
 * The ray of the integer pixel q of view v: d = Rp_v^T ((q.x - cx_v) / fx_v,
 * (q.y - cy_v) / fy_v, 1), d[k] = Rp[k] u + Rp[3 + k] w + Rp[6 + k] (step 4 of
 * mvs_wexp_children); it has camera z = 1, so a parameter along it is a depth.
 *
 * mvs_wdepth_splat_device: n patches, n < 2^31 (c, nrm, ref, mask), radius R in
 * 0..3, slope finite and > 0.  For every live patch p and every v in T(p)
 * inside the range:
 *   1. (x, y, z) = projection of c_p into v; skipped unless z > 0, 0 <= x < W
 *      and 0 <= y < H.  z = Rp_v[6] X + Rp_v[7] Y + Rp_v[8] Z + t_v[2], the
 *      filter's z_p(v).
 *   2. Skipped unless nrm_p.(O_v - c_p) > 0 (the difference first, then the dot
 *      product left to right): a back-facing patch draws nothing.
 *   3. (x0, y0) = (int(x + 0.5), int(y + 0.5)); the footprint is the integer
 *      pixels q with |q.x - x0| <= R and |q.y - y0| <= R inside the image.
 *   4. For each q: den = nrm_p.d(q), s = (nrm_p.(c_p - O_v)) / den; skipped
 *      unless den != 0, s is finite and > 0 and |s - z| <= slope (m + 1) z /
 *      ((fx_v + fy_v) / 2) with m = max(|q.x - x0|, |q.y - y0|), the right side
 *      evaluated left to right: a depth change of `slope` pixel footprints per
 *      pixel, which removes the blow-up of grazing planes.  s is the depth of
 *      the patch plane at q.
 *   5. zmap[v][q] (binary64) = the least s over all contributions, idmap[v][q]
 *      (int32) = the lowest p among those with exactly that s.  A pixel nobody
 *      reaches holds +inf and -1.
 * Every element of both maps is written (n = 0 still fills them): k_wdepth_fill,
 * then k_wdepth_splat twice -- a 64-bit atomic min of s's bit pattern, then an
 * unsigned 32-bit atomic min of the index among the holders of the minimum
 * (mvs_wfilt_front's idiom; the result does not depend on scheduling).  One
 * wave per patch; the (view, footprint pixel) pairs of a patch are flattened
 * over the lanes, 64 per pass.
 *
 * mvs_wdepth_consist_device: a zmap as given (it need not come from the splat),
 * rel_tol finite and >= 0; cons and viol are uint8 per pixel (viol may be
 * NULL).  For a pixel (v, q) whose z = zmap[v][q] is finite and > 0:
 *   1. X = O_v + z d(q), each component one product and one sum.
 *   2. For every other view u of the range, ascending: (x, y, depth) =
 *      projection of X into u; u is skipped unless depth > 0, x >= 0, y >= 0,
 *      int(x + 0.5) < W and int(y + 0.5) < H.
 *   3. zu = zmap[u][int(y + 0.5)][int(x + 0.5)].  A zu that is not finite
 *      (a hole, or nan) is unknown and counts nowhere.
 *   4. (v, q) is consistent with u when |zu - depth| <= rel_tol depth, and a
 *      violation (u sees through X) when zu - depth > rel_tol depth; a smaller
 *      zu is an occlusion and counts nowhere.  rel_tol depth is one product.
 * cons = the number of consistent views, viol = the number of violations; every
 * other pixel gets 0 and 0.  V <= 256, so a count never saturates.  One thread
 * per pixel (k_wdepth_consist), the other views a wave-uniform loop.
 *
 * mvs_wdepth_points_device: m listed pixels, m < 2^31, as int32 triples (v, q.x,
 * q.y) inside the range and the image.  xyz[3k..] = X as above from zmap[v][q]
 * and rgb[3k..] = the 3 bytes of the resident RGB image of view v at q; a pixel
 * whose z is not finite and > 0 yields nan (the quiet nan 0x7ff8000000000000)
 * and 0.  The device call reads nothing for a triple outside the range or the
 * image and writes nan and 0; the host-pointer call refuses it.  m = 0 returns
 * MVS_OK and launches nothing (k_wdepth_points, one thread per pixel).
 *
 * MVS_E_ARG (message in mvs_last_error) for a scalar out of range, a NULL
 * pointer (the patch rows may be NULL when n = 0, the pixel rows when m = 0),
 * n or m < 0 or >= 2^31, or a view range outside 0..V-1.  The host-pointer
 * variants are synchronous, on the context's stream and the staging buffer
 * that every host-pointer call of the context shares.  Stream-ordered (NULL =
 * the context's stream). */
int mvs_wdepth_splat_device(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm,
                            const int32_t* d_ref, const uint64_t* d_mask, int radius, double slope, int v0,
                            int nv, double* d_zmap, int32_t* d_idmap, void* stream);
int mvs_wdepth_splat(mvs_ctx* ctx, int64_t n, const double* c, const double* nrm, const int32_t* ref,
                     const uint64_t* mask, int radius, double slope, int v0, int nv, double* zmap,
                     int32_t* idmap);
int mvs_wdepth_consist_device(mvs_ctx* ctx, const double* d_zmap, int v0, int nv, double rel_tol,
                              uint8_t* d_cons, uint8_t* d_viol, void* stream);
int mvs_wdepth_consist(mvs_ctx* ctx, const double* zmap, int v0, int nv, double rel_tol, uint8_t* cons,
                       uint8_t* viol);
int mvs_wdepth_points_device(mvs_ctx* ctx, int64_t m, const int32_t* d_pix, const double* d_zmap, int v0,
                             int nv, double* d_xyz, uint8_t* d_rgb, void* stream);
int mvs_wdepth_points(mvs_ctx* ctx, int64_t m, const int32_t* pix, const double* zmap, int v0, int nv,
                      double* xyz, uint8_t* rgb);
/* ---- Per-pixel plane propagation on depth and normal maps ----
 * (no reference counterpart).  One sweep of a PatchMatch-style densification of
 * the maps that mvs_wdepth_splat draws: every pixel scores its own plane, the
 * planes of four neighbours extended to it and a small depth x normal grid
 * around its own plane against the plane-warped photo test, and takes the best.
 * A sweep is Jacobi style: it reads one set of maps and writes another, so the
 * result does not depend on any order of execution.  Cameras, rays, gray
 * values, the window, the bilinear form and the ncc are mvs_score_warped's;
 * the ray d_q of the integer pixel q and the centre O_v are the depth maps'
 * above (camera z of d is 1, so a map value is the camera depth).
 * Inputs, over the view range v0 .. v0 + nv - 1, laid out [v - v0][y][x]:
 * zmap binary64 (nv H W; a depth is a finite value > 0, anything else is
 * empty) and nmap binary64 (nv H W 3; the plane normal towards the cameras,
 * NOT normalised or checked; a nan component makes the pixel empty).  lists is
 * a HOST array int32 (nv, tv), tv in 1..32: row k is the list of views that the
 * pixels of view v0 + k are matched against -- absolute view numbers in
 * 0..V-1 (they need not lie in the range), distinct, none equal to the row's
 * own view, -1 only at the end; |T| = the number of entries >= 0.  Both calls
 * validate the lists.  Scalars: wid in 1..5, min_cos in [0, 1), min_ncc not
 * nan, top_k in 1..tv, step in 1..64, kd in 0..3, ka in 0..2, astep >= 0 in
 * radians, depth_px finite and > 0, step_scale > 0, ka astep step_scale <= 1.2.
 * Outputs, each written whole, none overlapping an input or another output:
 * z_out (nv H W), n_out (nv H W 3), score (nv H W) binary64, best int32
 * (nv H W), and scores binary64 (nv H W HY; may be NULL).
 * Per pixel q of view v of the range:
 *   1. Pixel test.  The window [q.x-wid, q.x+wid] x [q.y-wid, q.y+wid] must lie
 *      inside the image and its gray values a must not be constant (N sum a^2 -
 *      (sum a)^2 > 0); otherwise the pixel comes out empty.  The window is the
 *      integer pixels around q: nothing is projected into v.
 *   2. Hypotheses, HY = 5 + (2 kd + 1)(2 ka + 1)^2 planes (z_h, n_h) through
 *      X_h = O_v + z_h d_q (each component one product and one sum):
 *      h = 0 is the pixel's own plane (z, n); it exists when the pixel is not
 *      empty.
 *      h = 1..4 are the planes of the pixels (q.x-step, q.y), (q.x+step, q.y),
 *      (q.x, q.y-step), (q.x, q.y+step) extended to q: with the neighbour's
 *      (z', n') and ray d', z_h = (z' (n'.d')) / (n'.d_q), the dot products
 *      left to right and unfused, n_h = n' bit for bit.  The hypothesis does
 *      not exist when the neighbour lies outside the image or is empty, when
 *      the denominator is 0, or when z_h is not finite and > 0.  A neighbour
 *      within wid of the border is a valid source.
 *      h = 5 + ((k + kd) A + (j + ka)) A + (i + ka), A = 2 ka + 1, k = -kd..kd,
 *      i, j = -ka..ka is the refinement grid around the own plane; it exists
 *      only when h = 0 does.  dz = (depth_px z) / ((fx_v + fy_v) / 2),
 *      z_h = z + ((double)k dz) step_scale, and n_ij is exactly step 2 of
 *      mvs_refine_warped with nrm = n (the tangents from the host's libm,
 *      n_00 = n as given).  The grid's centre entry (k = i = j = 0) is h = 0
 *      again: it is never scored and its scores entry is nan.
 *   3. Score of an existing hypothesis.  It is invalid unless n_h.(O_v - X_h) >
 *      min_cos |O_v - X_h|.  For each list view u, in list order, ncc_u comes
 *      from steps 3-6 of mvs_score_warped with (n_h, X_h): the facing test,
 *      every window sample with positive depth and inside u, a warped window
 *      that is not constant; ncc_u is nan when any of these fails.  A view
 *      passes when ncc_u > min_ncc, and the hypothesis is valid when at least
 *      top_k views pass.  score_h = (the sum of the top_k largest passing ncc,
 *      added in descending order, equal values in list order) / top_k.  Every
 *      hypothesis thus averages the same number of terms, and an occluded list
 *      view costs nothing as long as top_k others see the plane.
 *   4. Choice, the refinement's rule.  The own plane is kept unless another
 *      valid hypothesis scores strictly higher; among the others the highest
 *      score wins, ties go to the lowest h.  best = the chosen h, score = its
 *      score (the same bits as scores[.. best]), z_out and n_out = its (z_h,
 *      n_h) -- for h = 0 the inputs bit for bit.  With no valid hypothesis or
 *      a failed pixel test: best -1, z_out +inf, n_out and score nan, every
 *      scores entry nan.  So a sweep is also a per-pixel photo check: a depth
 *      that no top_k views confirm is removed, and a pixel within wid of the
 *      border holds nothing afterwards.
 * Binary64 throughout; results are deterministic.  Geometry outside the sample
 * loop is left to right and unfused; the sample positions use k_refine_warp's
 * homogeneous form.  nv H W = 0 returns MVS_OK and launches nothing.
 * MVS_E_ARG (message in mvs_last_error) for a scalar out of range, a NULL
 * required pointer, a bad list, a view range outside 0..V-1 and overlapping
 * arrays.  The call reads the scene and its arguments only (k_wprop_sweep, one
 * launch per view, the view's list in the kernel arguments): no scorer
 * scratch, no counter sets, no atomics, no context state.  It may be
 * interleaved with every other call.  Device pointers, stream-ordered (NULL =
 * the context's stream). */
int mvs_wprop_sweep_device(mvs_ctx* ctx, int v0, int nv, const double* d_zmap, const double* d_nmap,
                           const int32_t* lists, int tv, int wid, double min_cos, double min_ncc, int top_k,
                           int step, int kd, int ka, double astep, double depth_px, double step_scale,
                           double* d_z_out, double* d_n_out, double* d_score, int32_t* d_best,
                           double* d_scores, void* stream);
/* Same on host pointers; synchronous, on the context's stream and the staging
 * buffer that every host-pointer call of the context shares. */
int mvs_wprop_sweep(mvs_ctx* ctx, int v0, int nv, const double* zmap, const double* nmap, const int32_t* lists,
                    int tv, int wid, double min_cos, double min_ncc, int top_k, int step, int kd, int ka,
                    double astep, double depth_px, double step_scale, double* z_out, double* n_out,
                    double* score, int32_t* best, double* scores);
/* ---- A surface from the depth maps: signed-distance fusion and marching
 * tetrahedra ----
 * (no reference counterpart).  Every view's depth map votes into one lattice of
 * truncated signed distances, and the surface is extracted once from it as an
 * indexed triangle mesh: the views are merged by construction.  Cameras,
 * "projection" and the maps' layout [v - v0][y][x] over a view range are the
 * depth maps' above; integer coordinates are pixel centres and a depth is the
 * camera z that the splat writes.  Binary64, products and sums left to right,
 * unfused, so every output is defined to the bit; tests/mesh_reference.py
 * restates both calls in Python floats.
 *
 * The lattice: (nx + 1)(ny + 1)(nz + 1) points, nx, ny, nz >= 1, at most 2^27
 * of them; P(i, j, k) = origin + (i, j, k) voxel, each coordinate one product
 * ((double)i voxel) and one sum; the point's linear index is (k (ny + 1) +
 * j)(nx + 1) + i, which is the layout of every lattice array.  origin is a host
 * array of 3 finite doubles, voxel is finite and > 0.
 *
 * mvs_wtsdf_integrate_device: trunc finite and > 0, min_weight >= 1.  For each
 * lattice point P, D = 0, Wt = 0, cnt = 0 and three integer sums = 0, then for
 * the views v = v0 .. v0 + nv - 1 in that order:
 *   1. (x, y, z) = projection of P into v; skipped unless z > 0, x >= 0, y >= 0,
 *      x + 0.5 < W and y + 0.5 < H (tested before the conversion, so nan and
 *      huge values never reach an integer: mvs_wdepth_consist's rule); the
 *      nearest pixel is q = (int(x + 0.5), int(y + 0.5)).
 *   2. zu = zmap[v][q]; skipped unless zu is finite and > 0.
 *   3. sdf = zu - z; skipped when sdf < -trunc (P is hidden behind the surface).
 *   4. r = sdf / trunc; D += (r < 1 ? r : 1); Wt += 1.
 *   5. When |sdf| <= trunc: the three bytes of the resident RGB image of v at q
 *      are added to the sums and cnt += 1.
 * tsdf[P] (binary64) = D / (double)Wt when Wt >= min_weight, else the quiet nan
 * 0x7ff8000000000000; weight[P] (int32) = Wt; rgb[P] (3 bytes) = (2 sum + cnt) /
 * (2 cnt) per channel in integer arithmetic, 0 when cnt = 0; cnt[P] (uint8) =
 * min(cnt, 255).  Every element of the four arrays is written.  The call keeps
 * no context state and reads the scene and its arguments only, so it runs on
 * any stream beside any other call.  k_wtsdf_integrate: one thread per lattice
 * point, a workgroup owns a brick of 16 x 4 x 4 points with i fastest (bricks
 * past the lattice's end are cut, so no size is special); the view loop is
 * wave-uniform with the camera in scalar registers; no atomics: the sum is in
 * view order.
 *
 * mvs_wmesh_extract_device: marching tetrahedra over a lattice of values tsdf
 * (as given; it need not come from the integration), with rgb and cnt per point.
 * Cube (i, j, k), 0 <= i < nx .., has the linear index (k ny + j) nx + i and the
 * corners P(i + a, j + b, k + c), a, b, c in {0, 1}.  It is cut into the six Kuhn
 * tetrahedra, one per permutation pi of the axes (0, 1, 2) in lexicographic
 * order (012, 021, 102, 120, 201, 210): corners c0 = (0,0,0), c1 = c0 + e_pi0,
 * c2 = c1 + e_pi1, c3 = (1,1,1).  Neighbouring cubes agree on every face
 * diagonal, there is no ambiguous case, and every edge of a tetrahedron runs
 * from a lattice point p to p + delta, delta in {0,1}^3 \ {0}: p, the lower
 * endpoint, owns the edge, whose type is delta.x + 2 delta.y + 4 delta.z - 1
 * (0..6).
 *   - A corner is inside when its value is < 0 (0.0 and -0.0 are outside).  A
 *     tetrahedron draws only when its four values are finite and it has inside
 *     and outside corners.
 *   - One inside corner a, or one outside corner a: one triangle, the edges from
 *     a to the other three corners in the tetrahedron's corner order.  Two
 *     inside corners a < b, outside c < d: the triangles (ac, ad, bd) and (ac,
 *     bd, bc).  A triangle's second and third vertex are then swapped where
 *     needed so that (p1 - p0) x (p2 - p0) points from the inside corners to the
 *     outside ones (a table of one bit per (tetrahedron, inside mask)).
 *   - A vertex exists exactly for the lattice edges that some drawn triangle
 *     uses; both tetrahedra that share an edge name the same vertex.  On the
 *     edge from a (the owner) to b: t = f_a / (f_a - f_b), position P_a + t (P_b -
 *     P_a) per coordinate, colour = rgb of a when t < 0.5, else of b; when that
 *     endpoint has cnt = 0, of the other one.
 *   - Exact zeros give triangles of zero area (all three vertices at one lattice
 *     point); they are kept.
 *   - Vertices are ordered by (owner's linear index, edge type), triangles by
 *     (cube's linear index, tetrahedron, triangle); indices are int32.
 * Sizing is mvs_wseed_match_device's: d_total[0] = the number of vertices and
 * d_total[1] = the number of triangles (int64, device), whatever the caps; the
 * first min(cap_v, total) vertices go to d_vert (binary64 x 3) and d_vcol (3
 * bytes), the first min(cap_t, total) triangles to d_tri (int32 x 3; an index
 * may name a vertex at or past cap_v), and nothing is written past a cap.
 * cap_v = cap_t = 0 counts only (the outputs may then be NULL).  Two runs are
 * bit-identical.  Passes: k_wmesh_mark (one thread per cube: the triangle count,
 * and an atomic OR of the used-edge bits into the owners' masks -- an OR does
 * not depend on the order of arrival), k_wmesh_vcount, k_wmesh_scan (exclusive
 * offsets of the workgroups' counts), k_wmesh_vertex and k_wmesh_tri (the mark
 * pass's arithmetic again; offsets inside a workgroup come from a scan in the
 * workgroup).  The masks (a byte per point), the points' first vertices (int32)
 * and the workgroups' counts live in the context's scratch, 5 bytes per point:
 * consecutive calls on one stream follow each other in stream order, and a
 * call on another stream waits for the previous call's work through an event
 * (as the expansion's grids do), so calls of one context never overlap.
 *
 * MVS_E_ARG (message in mvs_last_error) for a scalar out of range, nan or inf
 * (nx, ny, nz, origin, voxel, trunc, min_weight, cap_v or cap_t < 0 or >= 2^31),
 * a NULL required pointer, a view range outside 0..V-1 or more than 2^27
 * lattice points.  The host-pointer variants are synchronous, on the context's
 * stream and the staging buffer that every host-pointer call of the context
 * shares; they copy cap_v and cap_t whole entries back, of which those past the
 * totals are unspecified.  Stream-ordered (NULL = the context's stream). */
int mvs_wtsdf_integrate_device(mvs_ctx* ctx, const double* d_zmap, int v0, int nv, int nx, int ny, int nz,
                               const double* origin, double voxel, double trunc, int min_weight, double* d_tsdf,
                               int32_t* d_weight, uint8_t* d_rgb, uint8_t* d_cnt, void* stream);
int mvs_wtsdf_integrate(mvs_ctx* ctx, const double* zmap, int v0, int nv, int nx, int ny, int nz,
                        const double* origin, double voxel, double trunc, int min_weight, double* tsdf,
                        int32_t* weight, uint8_t* rgb, uint8_t* cnt);
int mvs_wmesh_extract_device(mvs_ctx* ctx, int nx, int ny, int nz, const double* origin, double voxel,
                             const double* d_tsdf, const uint8_t* d_rgb, const uint8_t* d_cnt, int64_t cap_v,
                             int64_t cap_t, double* d_vert, uint8_t* d_vcol, int32_t* d_tri, int64_t* d_total,
                             void* stream);
int mvs_wmesh_extract(mvs_ctx* ctx, int nx, int ny, int nz, const double* origin, double voxel, const double* tsdf,
                      const uint8_t* rgb, const uint8_t* cnt, int64_t cap_v, int64_t cap_t, double* vert,
                      uint8_t* vcol, int32_t* tri, int64_t* total);
/* CellTable.filter_out_outlier (MVS2.py:132-158) on the host, over n accepted
 * patches in fill order (what the stage's opt-in filter mode runs between
 * the expansion and reconstruct_from_Q): patch e has cell[2e..2e+1] =
 * which_cell of its projection (MVS2.py:113), mask[e*words..] its V list,
 * count[e] = |V|, avg[e] = avg_ncc_score, c[3e..], nrm[3e..].  Out:
 * alive[e] = 0 for the removed patches, stats[0] = removed patches,
 * stats[1] = "remove a outlier" lines the reference prints.  The
 * reference's ZeroDivisionError (a filled cell emptied before its visit,
 * MVS2.py:144) is MVS_E_DIVZERO.  Host pointers; no GPU needed. */
int mvs_filter_outliers(int64_t n, int words, int nci, int ncj, const int32_t* cell,
                        const uint64_t* mask, const int32_t* count, const double* avg,
                        const double* c, const double* nrm, uint8_t* alive, int64_t* stats);
/* The multi-GPU sweep's exchange record set (no reference counterpart: the
 * reference is single-process).  The accepted candidates
 * (count >= vlb, MVS2.py:256/369) of a slice of n scored candidates are
 * packed into d_out[(cap + 1) * width] int64 with width = 1 + words +
 * (d_c ? 3 : 0): row 0 = [accepted, n, 0...], rows 1.. = [offset + i, mask
 * words of i, and with d_c (the slice's n*3 centres, the candidates' 3D
 * points) the binary64 bits of x, y, z] (40 B at V <= 64; d_c = NULL: 16 B,
 * the receiver regenerating a point from its global index).  Row order: each
 * chunk of 8,192 candidates in index order, the chunks in the order they
 * reserve their rows (one atomic each; nothing waits for another chunk), so
 * the set is exact and the order is not: a receiver that needs index order
 * sorts by the first column (parallel.PointsExchange.result does).
 * d_count = NULL: d_mask is mvs_score_device_rec's records (words + 1 int64
 * each) and |V| their popcount.
 * Device pointers, stream-ordered, no host synchronisation (the accepted
 * total is in the header; a slice with more than cap accepted keeps cap of
 * them).  Calls on one context are ordered across streams (their counter is
 * the context's).  Feeds the all-gather of parallel.PointsExchange. */
int mvs_pack_accepted(mvs_ctx* ctx, int64_t n, int64_t offset, const int32_t* d_count,
                      const uint64_t* d_mask, const double* d_c, int vlb, int64_t cap, int64_t* d_out,
                      void* stream);
/* Measurement only (bench.py exchange.overlap_proxy): copies bytes (a
 * multiple of 16) from d_src to d_dst with a kernel of `workgroups`
 * 256-thread workgroups on `stream` -- the CU footprint of a collective's
 * kernel, run beside the scoring kernels on one GPU. */
int mvs_proxy_copy(void* d_dst, const void* d_src, int64_t bytes, int workgroups, void* stream);
/* The persistent tiled scorers' grid: `workgroups` > 0 holds them to that
 * many workgroups (at two per CU, the CUs of a CU-masked scoring stream), 0
 * restores the default (every CU, twice).  Multi-GPU steps score on a stream
 * whose CU mask leaves a few CUs to the exchange's pack and RCCL's kernels
 * (parallel.cu_masked_stream); no reference counterpart. */
int mvs_set_scorer_grid(mvs_ctx* ctx, int workgroups);
/* Kernel timing (measurement only): while enabled, every enable-th scoring
 * call (enable = 1: every call) records a HIP event pair on its stream
 * immediately around the dominant scoring kernel (k_score_mma / k_score_mma_v
 * for batches of >= 2048 candidates, else k_score); sampling keeps the
 * events' own stream time out of most calls of a timed loop.  enable > 0
 * resets the record and turns it on; 0 turns it off (the record stays
 * readable).  mvs_kernel_time synchronises the recorded events and returns
 * the summed kernel time and the number of timed launches; mvs_timed_kernel
 * names the kernel the last recorded pair bracketed. */
int mvs_kernel_timing(mvs_ctx* ctx, int enable);
int mvs_kernel_time(mvs_ctx* ctx, double* total_ms, int64_t* launches);
const char* mvs_timed_kernel(const mvs_ctx* ctx);
/* Number of per-view NCC decisions that fell inside the direct scorer's guard
 * band around the threshold (relative 1e-11 on the squared comparison; 1e-9
 * absolute when min_ncc < 0.01) and were re-evaluated in numpy order since the
 * context was created.  (The tiled scorer's own band, 2e-6 relative on its
 * binary32 comparison, sends a candidate to the direct scorer.) */
int64_t mvs_exact_hits(mvs_ctx* ctx);
/* A caller stream that a *_device call has used is about to be destroyed
 * (hipStreamDestroy): the context waits for that stream's work on its
 * scratch and pack areas now.  The context orders calls made on different
 * streams by an event recorded lazily on the stream that used an area last,
 * when the next call comes from another stream; a destroyed stream cannot
 * take that record (its handle may even be reused by a new stream), so a
 * caller that retires streams calls this first, on every context the stream
 * has used (parallel.MaskedStream.close does).  Streams the caller keeps
 * need nothing. */
int mvs_stream_retiring(mvs_ctx* ctx, void* stream);

/* Direct-path statistics of the tiled scorers since the context was created
 * (device work ordered before this call on the context's stream is counted;
 * call after synchronising the streams that scored): out[0] = candidates
 * re-scored by the direct path (k_score_fix: the tiled scorer's guard band
 * plus bucket overflow), out[1] = of them bucket overflow, out[2] = tiled
 * batches.  Diagnostic (bench.py reports the guard-band rate per sweep). */
int mvs_scorer_stats(mvs_ctx* ctx, int64_t* out);

/* Tiled batches since the context was created whose candidates were binned
 * into workgroup-private sorted runs (no global atomics) rather than into the
 * atomic tile buckets: dense batches of the tables scorer (V <= 64) of at most
 * 256 binning workgroups (2^20 candidates).  Environment, read when the context
 * is created: MVS_BIN=atomic keeps the atomic buckets everywhere;
 * MVS_BIN_RUNS_MAX=<k> lowers the workgroup limit. */
int64_t mvs_bin_runs_batches(mvs_ctx* ctx);

/* ctNcc (MVS2.py:39-43) on n explicit window pairs of npx (<= 128) uint8
 * pixels each (device pointers).  ncc[i] = closed-form value (numpy-order
 * value if force_exact or within 1e-9 of thr; nan for a constant window);
 * pass[i] = ncc > thr. */
int mvs_ncc_windows(int64_t n, int npx, const uint8_t* d_a, const uint8_t* d_b, double thr,
                    int force_exact, double* d_ncc, uint8_t* d_pass, void* stream);

/* DensePointsWithMVS2 (MVS2.py:176-295) without file IO: seeding from the SfM
 * tracks (MVS2.py:205-260), patch_expansion (MVS2.py:308-404, FIFO capped at
 * min(max_pops, 100000) pops) and reconstruct_from_Q ordering
 * (MVS2.py:159-173).  Tracks: track t owns observations
 * [track_off[t], track_off[t+1]); obs_view = image index, obs_xy = (x, y)
 * float32 pairs (GlobalSet point2d_list); element 0 is the reference view.
 * cell_size / scale / wid as args.cell_size, args.scale and the photo test's
 * window half-width (5 in the reference). */
int mvs_stage_run(mvs_ctx* ctx, int64_t n_tracks, const int64_t* track_off,
                  const int32_t* obs_view, const float* obs_xy, int cell_size, double scale,
                  int wid, int64_t max_pops, mvs_stage_result** out);
/* which = 0: initial_patches rows, 1: all_patches rows (x,y,z,r,g,b float64).
 * The rows are ordered and gathered on the device; mvs_stage_rows copies them
 * into a host buffer, mvs_stage_rows_device into a device buffer
 * (stream-ordered). */
int64_t mvs_stage_count(const mvs_stage_result* res, int which);
int mvs_stage_rows(const mvs_stage_result* res, int which, double* rows);
int mvs_stage_rows_device(const mvs_stage_result* res, int which, double* d_rows, void* stream);
/* stats[0..7] = pops, reference-equivalent photo tests, accepted patches,
 * queue entries left, candidates scored on the GPU, sweeps, seed candidates,
 * exact-path decisions. */
int mvs_stage_stats(const mvs_stage_result* res, int64_t* stats);
/* Host wall seconds per stage phase: times[0] seeding, [1] ordered commit and
 * sweep planning, [2] GPU sweeps, [3] sweep copy-back, [4] output ordering,
 * [5] the whole call. */
int mvs_stage_times(const mvs_stage_result* res, double* times);
void mvs_stage_free(mvs_stage_result* res);

/* Stage options of a context, for the stage runs that follow (mvs_stage_run,
 * mvs_stage_begin ... mvs_stage_finish).  MVS_STAGE_FILTER_OUTLIERS runs
 * CellTable.filter_out_outlier (MVS2.py:132-158) between the expansion and the
 * reconstruction, as if the reference's commented-out call at MVS2.py:281
 * were enabled (avg_ncc_score then follows the reference's arithmetic
 * exactly).  A filled cell whose patches were all removed before it is
 * visited makes the reference raise ZeroDivisionError: MVS_E_DIVZERO. */
#define MVS_STAGE_FILTER_OUTLIERS 1
/* avg_ncc_score (MVS2.py:62-76) in the reference's own arithmetic for n scored
 * candidates (host arrays: ref, xy (n*2) and mask (n*words) as mvs_score
 * returned them): ctNcc in numpy's order for every view of the mask, summed
 * in view order from 0, divided by the view count (0 for an empty mask).
 * mvs_score's avg agrees with it to 1e-12; this one is bit-exact. */
int mvs_exact_avg(mvs_ctx* ctx, int64_t n, const int32_t* ref, const double* xy, const uint64_t* mask,
                  int wid, double* avg);
int mvs_stage_set_options(mvs_ctx* ctx, int flags);
/* out[0] = outlier patches removed, out[1] = "remove a outlier" lines the
 * reference prints for them (|V|^2 each). */
int mvs_stage_filter_stats(const mvs_stage_result* res, int64_t* out);

/* The same stage in steps, for several GPUs (one process and one context per
 * GPU).  Every rank calls mvs_stage_begin with the same inputs
 * and its (rank, world), then loops:
 *   nj = mvs_stage_plan(st)          commit in reference order until the FIFO
 *                                    head needs unscored children; plan the next
 *                                    sweep of nj child jobs (0: stage finished)
 *   mvs_stage_score_slice(st, out)   the geometry of every child of the sweep
 *                                    (it depends only on parent records, which
 *                                    every rank holds) and the photo + accept
 *                                    test of this rank's contiguous slice
 *                                    (rank r: jobs [r*b + min(r, x),
 *                                    ... + b + (r < x)), b = nj / world,
 *                                    x = nj % world); the slice's photo-test
 *                                    masks go to the device buffer
 *                                    out[ceil(nj/world)][width] (world > 1;
 *                                    may be NULL when world == 1)
 *   <all-gather the slices, e.g. RCCL>
 *   mvs_stage_ingest(st, all)        all[world][ceil(nj/world)][width] (device):
 *                                    the other ranks' masks into the record
 *                                    table, their counts (popcount) and accept
 *                                    tests; `all` must be complete when called
 *                                    (the context's stream waits for no other
 *                                    stream)
 * and ends with mvs_stage_finish (same result as mvs_stage_run) and
 * mvs_stage_destroy.  width = mvs_stage_record_width(st) int64 words (the
 * mask words: 8 B per child at V <= 64).  Seeding
 * is replicated on every rank; the commit is identical on every rank because
 * it reads identical records.  Calls are synchronous. */
int mvs_stage_begin(mvs_ctx* ctx, int64_t n_tracks, const int64_t* track_off,
                    const int32_t* obs_view, const float* obs_xy, int cell_size, double scale,
                    int wid, int64_t max_pops, int rank, int world, mvs_stage** out);
int64_t mvs_stage_plan(mvs_stage* st);
int mvs_stage_record_width(const mvs_stage* st);
int mvs_stage_score_slice(mvs_stage* st, int64_t* d_out);
int mvs_stage_ingest(mvs_stage* st, const int64_t* d_all);
int mvs_stage_finish(mvs_stage* st, mvs_stage_result** out);
void mvs_stage_destroy(mvs_stage* st);

/* patch_expansion candidates (MVS2.py:329-369) for explicit jobs: job k =
 * (parent job_parent[k], hit view job_view[k], i = job_di[k] in {-1,+1}).
 * Parents: centre pc, normal pn, pxy = projection into the parent's
 * reference view (the x, y of its V entries).  Per job: X, nX (n of the new
 * patch), colour (img[int(cc1)][int(cc0)]), projection xy, mask/count of the
 * photo test at min_ncc, accept = |V| >= vlb && is_patch_neighbor(0.1) &&
 * |pc - X| < 0.05/scale.  Host pointers; wid 3 or 5. */
int mvs_expand_candidates(mvs_ctx* ctx, int64_t n_parents, const double* pc, const double* pn,
                          const double* pxy, int64_t n_jobs, const int32_t* job_parent,
                          const int32_t* job_view, const int32_t* job_di, int cell_size,
                          double scale, int wid, double min_ncc, double* X, double* nX,
                          uint8_t* color, double* xy, uint64_t* mask, int32_t* count,
                          uint8_t* accept);

/* Host geometry the stage uses, exported for parity tests:
 * cv2.Rodrigues round trip (utils.py:242-243) and cv2.triangulatePoints for one
 * point (utils.py:238-239, homogeneous 4-vector). */
int mvs_rodrigues_roundtrip(const double* R, double* Rp);
int mvs_triangulate(const double* P1, const double* P2, const double* x1, const double* x2,
                    double* X4);

/* ---- SfM front-end: the producer of the stage's seed tracks ----
 * (BASELINE config 5: HarrisFeatures + SFM.py feeding MVS; the reference's
 * default SfM matcher is OpenCV ORB/FLANN/RANSAC, SFM.py:56, utils.py:160-232)
 *
 * getHarrisPoints(imgs[view]) (HarrisFeatures.py:135-161) on the GPU:
 * cv2.cornerHarris(gray, 2, 3, 0.04), 3x3 dilate, keep > float32(0.01) * max,
 * np.where row-major order.  out: [col, row] int32 pairs (host), at most cap
 * of them; *n_out = the total (call with cap 0 to size the buffer). */
int mvs_harris_points(mvs_ctx* ctx, int view, int32_t* out, int64_t cap, int64_t* n_out);

/* MatchTwoSided(getDescFeatures(imgs[view_a], pts_a, wid),
 *               getDescFeatures(imgs[view_b], pts_b, wid), thr)
 * (HarrisFeatures.py:15-67) on the GPU.  pts_* are [row, col] int32 (host),
 * all inside getDescFeatures' bounds (else MVS_E_ARG).  m12[i] = j when j is
 * i's best match and i is j's, else -1; best12 / best21 (may be NULL): the
 * one-sided argmax of ncc > thr (ties -> smallest index, -1 when no ncc
 * exceeds thr; numpy's argsort leaves both cases implementation-defined). */
int mvs_match_two_sided(mvs_ctx* ctx, int view_a, const int32_t* pts_a, int64_t n_a, int view_b,
                        const int32_t* pts_b, int64_t n_b, int wid, double thr, int32_t* m12,
                        int32_t* best12, int32_t* best21);

/* One image pair of StructureFromMotion's loop (SFM.py:60-80), host:
 * P = K [R | t] per view (getProjectionMatrix), cv2.triangulatePoints of
 * the float32 correspondences q (view A) / tr (view B) (float32 result),
 * point = X / w; keep[i] = 1 when w != 0 and both projectPoint residuals
 * (float32 norm) are <= max_err (MIN_REPROJECTION_ERROR).  pt: float32 (n, 3).
 * K, R row-major 3x3, t 3 doubles. */
int mvs_sfm_pair(const double* KA, const double* RA, const double* tA, const double* KB,
                 const double* RB, const double* tB, int64_t n, const float* q, const float* tr,
                 double max_err, float* pt, uint8_t* keep);

#ifdef __cplusplus
}
#endif
#endif /* MVS_AMD_H */
