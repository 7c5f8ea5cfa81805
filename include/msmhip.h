/*
 * msmhip.h -- C ABI of libmsmhip.so, the MI355X (gfx950) engine behind the
 * pmarlo featurize -> TICA -> k-means -> transition-matrix -> ITS path.
 *
 * The reference (pmarlo, pure Python) has no FFI for this path: the seam is
 * "Python callables taking/returning numpy arrays" (SURVEY.md section 8b).  Each
 * entry point below therefore names the reference callable whose arithmetic it
 * replaces (file:line relative to the pmarlo tree, src/pmarlo = S/).  The
 * ctypes binding a pmarlo maintainer would add is shown in INTEGRATION.md and
 * implemented in pmarlo_amd/_lib.py.
 *
 * Conventions
 *   - every function returns an msm_status; 0 is success.  msm_last_error()
 *     gives the message for the last failure on that context.
 *   - pointers named d_* are DEVICE pointers (hipMalloc'ed, e.g. msm_malloc or
 *     a torch tensor's data_ptr()); pointers named h_* are HOST pointers.
 *   - matrices are row-major; `ld` is the row stride in ELEMENTS.
 *   - all work is enqueued on the context's HIP stream; nothing synchronises
 *     unless documented (msm_sync, msm_memcpy_d2h, functions with h_ outputs).
 *   - no torch / C++ types cross this boundary.
 */
#ifndef MSMHIP_H
#define MSMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct msm_ctx msm_ctx;
typedef struct msm_event msm_event;
typedef struct msm_graph msm_graph;

typedef enum {
    MSM_OK = 0,
    MSM_ERR_INVALID = 1,     /* bad argument            -> ValueError   */
    MSM_ERR_HIP = 2,         /* HIP runtime failure     -> RuntimeError */
    MSM_ERR_NOMEM = 3,       /* allocation failure      -> MemoryError  */
    MSM_ERR_UNSUPPORTED = 4, /* shape outside kernel limits -> NotImplementedError */
    MSM_ERR_NOCONV = 5       /* iterative solver did not converge -> RuntimeError */
} msm_status;

/* element type of a feature matrix handed to the engine */
typedef enum { MSM_F32 = 0, MSM_F64 = 1 } msm_dtype;

/* ------------------------------------------------------------------ */
/* context, memory, timing                                              */
/* ------------------------------------------------------------------ */

/* Create a context on HIP device `device`.  `hip_stream` may be NULL (the
 * context then owns a new non-blocking stream) or an existing hipStream_t
 * (e.g. torch.cuda.current_stream().cuda_stream) which is borrowed. */
msm_status msm_ctx_create(int device, void* hip_stream, msm_ctx** out);
void msm_ctx_destroy(msm_ctx* ctx);
const char* msm_last_error(const msm_ctx* ctx);
/* "gfx950" etc.; number of compute units; bytes of device memory */
msm_status msm_device_info(msm_ctx* ctx, char* arch, size_t arch_len,
                           int* n_cu, size_t* total_mem);
const char* msm_version(void);

msm_status msm_malloc(msm_ctx* ctx, size_t bytes, void** d_out);
msm_status msm_free(msm_ctx* ctx, void* d_ptr);
msm_status msm_memcpy_h2d(msm_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
msm_status msm_memcpy_d2h(msm_ctx* ctx, void* h_dst, const void* d_src, size_t bytes); /* syncs */
msm_status msm_memcpy_d2d(msm_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
msm_status msm_memset(msm_ctx* ctx, void* d_dst, int value, size_t bytes);
msm_status msm_sync(msm_ctx* ctx);

/* HIP events on the context's stream (bench.py times kernels with these). */
msm_status msm_event_create(msm_ctx* ctx, msm_event** out);
void msm_event_destroy(msm_event* ev);
msm_status msm_event_record(msm_ctx* ctx, msm_event* ev);
msm_status msm_event_elapsed_ms(msm_event* start, msm_event* stop, float* h_ms); /* syncs on stop */

/* Stream capture: everything enqueued between begin and end becomes one
 * hipGraph that msm_graph_launch replays (launch-bound inner loops). */
msm_status msm_graph_begin(msm_ctx* ctx);
msm_status msm_graph_end(msm_ctx* ctx, msm_graph** out);
msm_status msm_graph_launch(msm_ctx* ctx, msm_graph* g);
void msm_graph_destroy(msm_graph* g);

/* ------------------------------------------------------------------ */
/* featurizers                                                          */
/* ------------------------------------------------------------------ */

/* Per-frame geometry on d_xyz float32 [n, A, 3] (nm), written as float32 columns
 * [col_off, col_off + width) of d_out [n, ld].  fp32 arithmetic in the operation
 * order of the reference's in-repo extractor (S/features/deeptica/
 * ts_feature_extractor.py:423-500, use_pbc = False), which is also what stands in
 * for mdtraj.compute_distances / compute_dihedrals behind featurize_trajectory
 * (S/features/featurize.py:41-62), PhiPsiFeature / DistanceFeature / AngleFeature /
 * DihedralFeature (S/features/builtins.py:42-86, 281-395) and
 * FeaturesMixin._compute_phi_psi_features (S/markov_state_model/_features.py:131-142).
 *   distances: d_pairs int32 [P, 2]      d = sqrt(max(|x_j - x_i|^2, 1e-12))
 *   angles   : d_triplets int32 [T, 3]   acos(clamp(v1.v2 / (|v1||v2|), -1, 1)), vertex = middle atom
 *   dihedrals: d_quads int32 [Q, 4]      atan2 form, wrapped to (-pi, pi] (builtins.py:11-14)
 *       mode 0: Q columns of radians
 *       mode 1: 2Q columns [cos_0, sin_0, cos_1, sin_1, ...]  (trig_expand_periodic,
 *               S/api/features.py:138-180)
 *       mode 2: 2Q columns [cos_0..cos_{Q-1} | sin_0..sin_{Q-1}] (_features.py:131-142)
 * Non-finite coordinates follow the reference's torch operations (clamp_min and clamp keep NaN): a
 * distance or an angle that reads a NaN coordinate is NaN; a dihedral that reads one is 0 (the
 * extractor's mask |x| + |y| >= eps is false for NaN), i.e. (cos, sin) = (1, 0) in modes 1 and 2; a
 * lone infinite coordinate gives a +inf distance, a NaN angle and a dihedral of 0; inf - inf is NaN.
 * Records and frames that read no such coordinate are not affected. */
msm_status msm_featurize_distances(msm_ctx* ctx, const float* d_xyz, int64_t n, int A,
                                   const int32_t* d_pairs, int P, float* d_out, int64_t ld, int col_off);
/* contacts: 1.0 where the pair distance is <= rcut (nm), else 0.0; a NaN or infinite distance (a
 * non-finite coordinate of either atom) is "no contact", 0.0, as in the reference, which sets NaN to
 * inf before it compares.  Rg: radius of gyration with unit masses, one column, fp64 accumulation and
 * one rounding to fp32; NaN for a frame with any non-finite coordinate
 * (S/features/builtins.py:89-108, 252-275). */
msm_status msm_featurize_contacts(msm_ctx* ctx, const float* d_xyz, int64_t n, int A,
                                  const int32_t* d_pairs, int P, float rcut, float* d_out,
                                  int64_t ld, int col_off);
msm_status msm_featurize_rg(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, float* d_out,
                            int64_t ld, int col_off);
msm_status msm_featurize_angles(msm_ctx* ctx, const float* d_xyz, int64_t n, int A,
                                const int32_t* d_triplets, int Tn, float* d_out, int64_t ld, int col_off);
msm_status msm_featurize_dihedrals(msm_ctx* ctx, const float* d_xyz, int64_t n, int A,
                                   const int32_t* d_quads, int Q, int mode, float* d_out, int64_t ld,
                                   int col_off);

/* Periodic boundaries.
 *   msm_box_from_cell: d_cell float64 [n, 6] = a, b, c (nm), alpha, beta, gamma (degrees) -> d_box float32 [n, 9],
 *       rows a, b, c with a along x and b in the xy-plane (mdtraj's unitcell_vectors).  fp64 arithmetic, components
 *       within 1e-6 of zero set to zero as mdtraj does, one rounding to fp32.
 *   msm_featurize_spec: one launch for a mixed feature list, the arithmetic of the four entry points above with the
 *       reference extractor's minimum-image step (S/features/deeptica/ts_feature_extractor.py:414-501) in front.
 *       d_box: NULL (n_box = 0), or float32 [n_box, 9] with n_box = 1 (one box for every frame) or n_box = n.
 *       d_rec int32 [F, 8], 16-byte aligned, one record per feature; sort it by kind so waves stay converged:
 *           [0] kind      MSM_FEAT_DISTANCE (atoms 0, 1), _ANGLE (0, 1, 2; vertex 1), _DIHEDRAL (0..3), _CONTACT (0, 1)
 *           [1..4] atoms  indices into [0, A); unused slots 0
 *           [5] flags     MSM_FEAT_MIC: bond vectors are replaced by their minimum image (ignored without a box);
 *                         MSM_FEAT_COSSIN (dihedral): emit cos into column [6] and sin into column [7]
 *           [6] column    relative to col_off, in [0, width)
 *           [7] column of the sine for MSM_FEAT_COSSIN, else ignored
 *       d_param float32 [F]: the weight every emitted value is multiplied by (1 is exact), or rcut for a contact.
 *       width: columns [col_off, col_off + width) of d_out [n, ld] are the table's; col_off + width <= ld is checked
 *           here, and a record whose column lies outside [0, width) writes nothing.
 *       mic: MSM_MIC_ROUND   f = v B^-1, v' = (f - round(f)) B, the reference extractor's rule;
 *            MSM_MIC_SEARCH  additionally the 27 neighbouring images of v', shortest wins, lowest image index
 *                            9 (i + 1) + 3 (j + 1) + (k + 1) on a tie: mdtraj's rule for triclinic cells.  (A v'
 *                            shorter than 0.49 of the cell's smallest perpendicular width is the only shortest
 *                            image and is kept without trying the others.)
 *       B^-1 is the adjugate over the determinant in fp32, once per frame and block.  Without a box, or for an
 *       unflagged record, the result is bit for bit that of the per-kind entry points.  A frame whose box is not
 *       finite or has determinant 0 gets NaN in its flagged columns; so does a record with an unknown kind or an
 *       atom index outside [0, A), in every frame. */
#define MSM_FEAT_DISTANCE 0
#define MSM_FEAT_ANGLE 1
#define MSM_FEAT_DIHEDRAL 2
#define MSM_FEAT_CONTACT 3
#define MSM_FEAT_MIC 1
#define MSM_FEAT_COSSIN 2
#define MSM_MIC_ROUND 0
#define MSM_MIC_SEARCH 1
msm_status msm_box_from_cell(msm_ctx* ctx, const double* d_cell, int64_t n, float* d_box);
msm_status msm_featurize_spec(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const float* d_box,
                              int64_t n_box, const int32_t* d_rec, const float* d_param, int F, int width,
                              int mic, float* d_out, int64_t ld, int col_off);

/* The adjoint of msm_featurize_spec: d_gxyz[t, a, :] = sign * sum_f d_gfeat[t, col_off + col(f)] * d feature_f / d x_a,
 * float64 [n, A, 3], for the record table, box rules and mic modes above.  Used with sign = -1 on dE/dfeature it
 * gives the force on every atom.
 *   Bond vectors are the forward's: the same fp32 difference and the same minimum-image step, then widened to fp64;
 *   everything after that is fp64.  The image shift is piecewise constant, so a wrapped vector differentiates like a
 *   plain difference; there is no gradient with respect to the box.
 *   Jacobians are closed forms: distance v / |v|; angle -1 / sin(theta) d cos(theta), written on v1, v2 and v1 x v2
 *   (d theta / d v1 = v1 x (v1 x v2) / (|v1|^2 |v1 x v2|)); dihedral the four-atom formula on c0 = b0 x b1,
 *   c1 = b1 x b2 and |b1| (d phi / d x0 = -|b1| c0 / |c0|^2, d phi / d x3 = |b1| c1 / |c1|^2; the +2 pi wrap does not
 *   enter); MSM_FEAT_COSSIN: (g_cos * -sin(phi) + g_sin * cos(phi)) times the dihedral's Jacobian, with cos and sin
 *   taken from the forward's (x, y), no inverse trigonometry.  d_param[f] multiplies every Jacobian.  A contact is
 *   a step function and contributes nothing.
 *   Degenerate geometry: where the forward's floor, clamp or mask is active -- a squared norm at or below 1e-12,
 *   |cos(theta)| >= 1 (or v1 x v2 = 0), |x| + |y| < 1e-12 of a dihedral, all evaluated in this function's fp64
 *   arithmetic -- the feature contributes exactly zero.  DIVERGENCE from torch's autograd, which returns 0, inf or
 *   NaN there depending on the branch (sqrt at the floor, acos at the clamp, atan2 at the origin).
 *   A record with an unknown kind, a column outside [0, width), an atom outside [0, A), or a flagged record under a
 *   singular box contributes nothing (the forward wrote NaN there, and its consumer hands a NaN gradient back).
 *   A frame whose gradient block [col_off, col_off + width) holds a non-finite value gets NaN on ALL its atoms and
 *   disturbs no other frame.  NaN coordinates propagate into the atoms they reach.
 *   d_inc_ptr int32 [A + 1], d_inc int32 [d_inc_ptr[A]]: the atom -> (record, slot) incidence in CSR form, built
 *   once per table: atom a's entries are d_inc[d_inc_ptr[a] .. d_inc_ptr[a + 1]), each record * 4 + slot (slot: which
 *   of the record's atoms a is), in ascending order; at most 4 F entries in all.  One thread owns one (frame, atom),
 *   walks the atom's entries in that order and sums in fp64: no floating-point atomics, equal inputs give equal
 *   bits, and a frame's result depends neither on n nor on where the frame sits.  An entry naming a record outside
 *   [0, F), or a slot that is not atom a's, contributes nothing.  An atom without entries is written as 0.0: the
 *   whole block [n, A, 3] is written.
 * One plain launch on the context's stream, capturable. */
msm_status msm_featurize_spec_vjp(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const float* d_box,
                                  int64_t n_box, const int32_t* d_rec, const float* d_param, int F, int width,
                                  int mic, const double* d_gfeat, int64_t ldg, int col_off,
                                  const int32_t* d_inc_ptr, const int32_t* d_inc, double sign, double* d_gxyz);

/* Structure features whose reference implementation is an mdtraj algorithm (S/features/builtins.py:171-250: the
 * built-ins "sasa", "hbonds_count", "ssfrac", all three in the default feature set of S/api/features.py:378).
 *   sasa: Shrake-Rupley accessible area per atom, float32 [n, A] (nm^2), as mdtraj.shrake_rupley computes it
 *         (geometry/src/sasa.cpp) before its per-residue sums: d_radii float32 [A] = atomic radius + probe radius,
 *         d_points float32 [P, 3] = the unit sphere points (golden spiral), fp32 throughout.
 *   hbond presence: for every (donor, hydrogen, acceptor) row of d_triplets int32 [Tn, 3] the number of frames with
 *         |H - A| < dist_cutoff and angle(D, H, A) > angle_cutoff (radians), the two criteria of
 *         mdtraj.baker_hubbard (geometry/hbond.py); the frequency threshold is the caller's.  A triplet without an
 *         angle in a frame (D = H or H = A there) is absent in it, as in mdtraj.
 *   dssp: Kabsch-Sander secondary structure per frame and residue (mdtraj.compute_dssp, geometry/src/dssp.cpp):
 *         d_backbone int32 [R, 4] = atom indices of N, CA, C, O of each protein residue, d_chain int32 [R],
 *         d_proline uint8 [R]; d_codes uint8 [n, R]: 0 loop, 1 H, 2 B, 3 E, 4 G, 5 I, 6 T, 7 S.  A row of
 *         d_backbone that holds a -1 is a residue without a full backbone: never bonded, a chain break, code 0. */
msm_status msm_featurize_sasa(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const float* d_radii,
                              const float* d_points, int P, float* d_out);
msm_status msm_hbond_presence(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const int32_t* d_triplets,
                              int Tn, float dist_cutoff, float angle_cutoff, uint64_t* d_counts);
msm_status msm_dssp(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const int32_t* d_backbone,
                    const int32_t* d_chain, const uint8_t* d_proline, int R, uint8_t* d_codes);

/* Rigid-body superposition onto a reference (mdtraj Trajectory.superpose as align_trajectory calls it,
 * S/api/features.py:110-135) and the RMSD to it (the CV "RMSD_ref", S/api/feature_profiles.py:41-45).
 *   d_sel int32 [S]: the atoms the fit uses, indices into [0, A) (the caller checks the range);
 *   d_ref float32 [S, 3]: reference positions of those atoms, not centred;
 *   d_out float32 [n, A, 3] or NULL; it may equal d_xyz (in place) but must not overlap it otherwise;
 *   d_rmsd float32 [n] or NULL; at least one of the two.
 * Per frame, with x_i the selected atoms, c their mean and c_ref the mean of d_ref: R is the PROPER rotation
 * (det +1) minimising sum_i |R (x_i - c) - (r_i - c_ref)|^2;  out_a = R (x_a - c) + c_ref for all A atoms;
 * rmsd = sqrt(max(0, (G_x + G_r - 2 lambda) / S)), G the sums of squared centred coordinates, lambda the optimal
 * overlap.  Centroids, G and the 3 x 3 correlation matrix are fp64 sums of the fp32 inputs; R is the eigenvector of
 * the largest eigenvalue of Horn's 4 x 4 quaternion matrix by cyclic Jacobi in fp64 (at most 16 sweeps); R is
 * applied in fp32.  A zero correlation matrix (S = 1, coinciding atoms) gives R = identity; a degenerate largest
 * eigenvalue (collinear atoms, S = 2) gives one of the minimisers; a frame with a non-finite selected coordinate
 * gets NaN in all its outputs and disturbs no other frame.  Parity with mdtraj's fp32 QCP code is unpinned.
 * The launch is picked by shape alone:
 *   d_out given, A <= LDS_ATOMS: a workgroup holds min(TILE_FRAMES, TILE_FLOATS / (3 A)) frames in LDS between
 *       the accumulate and the apply pass (xyz read once, written once; 16-byte accesses where d_out has d_xyz's
 *       offset modulo 16 bytes, 4-byte stores otherwise);
 *   d_out given, A >  LDS_ATOMS: a workgroup per frame, which reads the frame twice;
 *   d_out NULL: only the S selected atoms of a frame are read;
 *   the accumulate pass uses 8 lanes per frame for S <= NARROW_SEL and a wave above; for given (S, inputs) the
 *   RMSD and the rotation have the same bits on every path. */
#define MSM_SUPERPOSE_TILE_FRAMES 64      /* most frames of one LDS tile */
#define MSM_SUPERPOSE_TILE_FLOATS 12288   /* coordinates of one LDS tile: 48 KiB; with the per-frame sums 28-60 KiB a workgroup */
#define MSM_SUPERPOSE_LDS_ATOMS 4096      /* TILE_FLOATS / 3: the largest frame that fits the tile */
#define MSM_SUPERPOSE_NARROW_SEL 64       /* largest S accumulated on 8 lanes per frame */
msm_status msm_superpose(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const int32_t* d_sel, int S,
                         const float* d_ref, float* d_out, float* d_rmsd);

/* ------------------------------------------------------------------ */
/* lag-tau transition counts                                            */
/* ------------------------------------------------------------------ */

/* Unweighted lag-tau transition counts over trajectory segments.
 * Replaces pmarlo.analysis.discretize._weighted_counts (S/analysis/
 * discretize.py:609-645, weights=None) and, with stride=1, the deeptime
 * "sliding" count of EstimationMixin._count_transitions_deeptime
 * (S/markov_state_model/_estimation.py:116-156) and
 * debug_export._build_transition_counts (S/analysis/debug_export.py:385-409).
 *
 * For every segment [start, stop) with stop-start > lag and every
 * t = start, start+stride, ... < stop-lag: if labels[t] and labels[t+lag] are
 * both in [0, k) then counts[labels[t]][labels[t+lag]] += 1.
 * (The reference keeps pairs with both labels >= 0; labels >= k cannot occur
 * there because k = max label + 1.  Here they are skipped, never written.)
 *
 * d_labels  int32 [n]           h_seg_start/h_seg_stop  int64 [n_seg] (clipped to [0,n])
 * d_counts  int64 [k*k]  OVERWRITTEN   d_pairs  int64 [1] OVERWRITTEN (may be NULL)
 */
msm_status msm_count_transitions(msm_ctx* ctx, const int32_t* d_labels, int64_t n,
                                 const int64_t* h_seg_start, const int64_t* h_seg_stop,
                                 int n_seg, int lag, int stride, int k,
                                 int64_t* d_counts, int64_t* d_pairs);

/* msm_count_transitions followed by msm_transition_matrix in mode 0 (d_T = counts / row sum with zero rows left zero,
 * d_rowsum [k], d_diag_mass = trace(T) / k), same values and bits.  Where the dense two-pass counting runs (unweighted,
 * pairs >= k^2, a bucket of rows fits the LDS) the workgroup that owns a bucket of rows normalises them before it lets
 * them go, and the one that finishes last adds up the diagonal: ONE launch less per step.  Every other case (sparse
 * pairs, large k, a capture that cannot grow the scratch) runs the two calls. */
msm_status msm_count_transitions_normalised(msm_ctx* ctx, const int32_t* d_labels, int64_t n,
                                            const int64_t* h_seg_start, const int64_t* h_seg_stop, int n_seg, int lag,
                                            int stride, int k, int64_t* d_counts, int64_t* d_pairs, double* d_T,
                                            double* d_rowsum, double* d_diag_mass);

/* Weighted variant: counts[src][dst] += w[t] (weight of the STARTING frame,
 * S/analysis/discretize.py:633-641).  d_counts is float64 [k*k]. The sum is
 * accumulated with fp64 atomics, so it equals the reference up to summation
 * order (exact whenever the weights are dyadic / integer valued). */
msm_status msm_count_transitions_weighted(msm_ctx* ctx, const int32_t* d_labels,
                                          const double* d_weights, int64_t n,
                                          const int64_t* h_seg_start, const int64_t* h_seg_stop,
                                          int n_seg, int lag, int stride, int k,
                                          double* d_counts, int64_t* d_pairs);

/* Lag scan: counts for n_lag lags in one launch (ITS scan,
 * S/markov_state_model/_its.py:525-541 called once per lag).
 * h_lags int32 [n_lag]; d_counts int64 [n_lag*k*k]; d_pairs int64 [n_lag]. */
msm_status msm_count_transitions_lagscan(msm_ctx* ctx, const int32_t* d_labels, int64_t n,
                                         const int64_t* h_seg_start, const int64_t* h_seg_stop,
                                         int n_seg, const int32_t* h_lags, int n_lag, int k,
                                         int64_t* d_counts, int64_t* d_pairs);

/* Which kernels a count of `total_pairs` pairs (the pair positions of all segments, valid labels or not) over k states
 * would run on this context NOW: a read-only query of the one dispatch function the four calls above go through.  It
 * launches and allocates nothing.  The answer depends on the device's CU count, on the MSM_COUNTS_CHUNK and
 * MSM_COUNTS_BUCKETS environment variables and, while a capture is active, on the auxiliary scratch the context
 * already holds (a capture cannot grow it: the privatised kernel runs instead of the bucket path).
 *   out[0] = MSM_COUNT_PATH_*
 *   BUCKET:      out[1] = R (rows of a bucket), out[2] = buckets, out[3] = chunk (pairs of a first-pass workgroup),
 *                out[4] = chunks, out[5] = copies of a bucket's bins, out[6] = 1 if msm_count_transitions_normalised
 *                normalises in the counting launch (it still needs k doubles of scratch for the diagonal, which a
 *                capture cannot grow either)
 *   PRIVATISED:  out[1] = rows of a row block, out[2] = row_blocks, out[3] = chunks, out[4] = pairs_per_chunk,
 *                out[5] = lds_bytes
 *   GLOBAL:      out[3] = chunks (workgroups)
 *   NONE:        no pairs, the outputs are only cleared
 * Entries not named are zero.  weighted != 0: msm_count_transitions_weighted. */
#define MSM_COUNT_PATH_BUCKET 0
#define MSM_COUNT_PATH_PRIVATISED 1
#define MSM_COUNT_PATH_GLOBAL 2
#define MSM_COUNT_PATH_NONE 3
msm_status msm_count_transitions_plan(msm_ctx* ctx, int k, int64_t total_pairs, int weighted, int64_t out[8]);

/* Visits per state: np.bincount(labels[0<=l<k], minlength=k)
 * (S/analysis/discretize.py:648-667, weights=None).  d_visits int64 [k].  Up to MSM_STATE_COUNTS_LDS_MAX_K states a
 * workgroup bins in its LDS; above, every frame is one global atomic. */
#define MSM_STATE_COUNTS_LDS_MAX_K 16384
msm_status msm_state_counts(msm_ctx* ctx, const int32_t* d_labels, int64_t n, int k,
                            int64_t* d_visits);

/* Dwell times (runs of one state) of a label sequence in which negative labels separate trajectories
 * (_compute_dwell_times, S/analysis/debug_export.py:447-530, after its removal of unassigned frames):
 * d_stats int64 [4][k] = {min, max, sum, number} of the run lengths per state (min = -1 for a state
 * without runs); every run is also appended, in no particular order, to d_run_state int32 / d_run_len
 * int64 [capacity] (for the medians; capacity >= number of runs, at most n), *d_n_runs = runs found. */
msm_status msm_run_lengths(msm_ctx* ctx, const int32_t* d_labels, int64_t n, int k, int64_t* d_stats,
                           int32_t* d_run_state, int64_t* d_run_len, int64_t capacity, int64_t* d_n_runs);

/* ------------------------------------------------------------------ */
/* standardisation moments, time-lagged covariance, TICA               */
/* ------------------------------------------------------------------ */

/* Column moments of X [n, ld].  Replaces the statistics half of
 * reduction._preprocess (S/markov_state_model/reduction.py:13-40: SimpleImputer
 * mean + StandardScaler, ddof = 0) and of _KMeansDiscretizer.fit
 * (S/analysis/discretize.py:446-447: np.mean / np.std(ddof=1)).
 * NaN entries are skipped (the reference imputes them with the column mean,
 * which leaves mean and the centred sum of squares unchanged except for the
 * divisor, see msm_moments_finalize).
 *
 * _partial writes raw sums d_sums = [cnt F][S1 F][S2 F] with S1 = sum(x-shift),
 * S2 = sum((x-shift)^2); d_shift NULL means "row 0 of X" (NaN -> 0) and the
 * shift used is returned in d_shift_out [F] (may be NULL).  Shards that share
 * one shift vector all-reduce d_sums by plain summation.
 * _finalize: mean = shift + S1/cnt, std = sqrt((S2 - S1^2/cnt)/(cnt - ddof)).
 * msm_column_moments = partial + finalize.  d_count [F] f64 may be NULL. */
msm_status msm_column_moments_partial(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F,
                                      int64_t ld, const double* d_shift, double* d_sums,
                                      double* d_shift_out);
msm_status msm_moments_finalize(msm_ctx* ctx, const double* d_sums, const double* d_shift, int F,
                                int ddof, double* d_mean, double* d_std, double* d_count);
/* The remaining column statistics of validate_features (S/analysis/validation.py:89-172): d_min / d_max [F] over the
 * finite entries of every column (NaN for a column without any), d_counts int64 [2] = {non-finite entries, rows that
 * are finite throughout}.  With msm_column_moments this replaces four host passes over the matrix. */
msm_status msm_column_minmax(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                             double* d_min, double* d_max, int64_t* d_counts);
msm_status msm_column_moments(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F,
                              int64_t ld, int ddof, double* d_mean, double* d_std, double* d_count);

/* mean / divisor / reciprocal divisor of reduction._preprocess (reduction.py:13-40) from the
 * raw sums, on the device (no host round trip between the moments and covariance passes):
 * mean = shift + S1/cnt; sigma = sqrt((S2 - S1^2/cnt)/n_rows) -- NaNs imputed with the
 * column mean count in n_rows (the total row count over all shards) -- and sigma < 10 eps
 * -> 1 (sklearn's zero-scale rule); with_std == 0 gives sigma = 1 (scale=False). */
msm_status msm_standardise_params(msm_ctx* ctx, const double* d_sums, const double* d_shift, int F,
                                  double n_rows, int with_std, double* d_mean, double* d_scale,
                                  double* d_inv_scale);

/* Raw time-lagged moments on the fp64 matrix cores.  Replaces the covariance
 * accumulation inside deeptime TICA.fit as called by reduction.tica_reduce
 * (S/markov_state_model/reduction.py:103-109) and FeaturesMixin._maybe_apply_tica
 * (S/markov_state_model/_features.py:194-202): per segment x = X[:-lag],
 * y = X[lag:] (pairs never cross segments), reversible estimator.
 * With z = x - shift (NaN -> 0, i.e. imputed to the column mean):
 *   d_moments = [M00 F*F][M0t F*F][sx F][sy F][T]   (2F^2 + 2F + 1 doubles)
 *   M00 = sum_{X0} z z' + sum_{Yt} z z',  M0t = sum_pairs z_t z_{t+lag}',
 *   sx / sy = column sums over X0 / Yt, T = number of pairs.
 * Un-normalised on purpose: shards all-reduce d_moments by summation
 * (they must share d_shift).  At most 16 segments per call.  F <= 64 runs the fused
 * single-pass kernel; larger F the 64 x 64 block-task kernel.
 * assume_finite != 0 skips the NaN test (callers know from msm_column_moments'
 * d_count whether X holds NaNs; with NaNs present it must be 0).
 * lag == 0 gives the instantaneous second moments (M00 = 2 sum z z', T = n): the covariance
 * behind pca_reduce (S/markov_state_model/reduction.py:43-74). */
msm_status msm_lagged_moments(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                              const int64_t* h_seg_start, const int64_t* h_seg_stop, int n_seg, int lag,
                              const double* d_shift, int assume_finite, double* d_moments);

/* The same pass with the M0t block SYMMETRISED: the slot holds (M0t + M0t') / 2, everything else as above.  That is
 * all the reversible estimator reads of M0t (deeptime forms C0t = (X'Y + Y'X) / 2T), and it is cheaper: for
 * 32 < F <= 64 the kernel accumulates S = sum_pairs (z_t + z_{t+lag})(z_t + z_{t+lag})' and M00, both symmetric
 * (2 x F(F+16)/2 multiply-adds per frame instead of F^2 + F(F+16)/2), and finishes with (S - M00) / 2; other shapes
 * run the plain pass and symmetrise in place.  Still additive over shards. */
msm_status msm_lagged_moments_reversible(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                                         const int64_t* h_seg_start, const int64_t* h_seg_stop, int n_seg, int lag,
                                         const double* d_shift, int assume_finite, double* d_moments);

/* The same pass with ONE-SIDED second moments: M00 = sum over X0 only (M0t, sx, sy, T as above).
 * What the reference's in-repo TICA eigenvalue estimator needs (separate means and covariance of
 * y_t: _estimate_top_eigenvalues, S/features/deeptica/core/trainer_api.py:641-646). */
msm_status msm_lagged_moments_onesided(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F,
                                       int64_t ld, const int64_t* h_seg_start, const int64_t* h_seg_stop,
                                       int n_seg, int lag, const double* d_shift, int assume_finite,
                                       double* d_moments);

/* _estimate_top_eigenvalues (S/features/deeptica/core/trainer_api.py:632-656) from one-sided moments:
 *   C0 = (M00 - sx sx'/T)/max(1, T-1), Ct = (M0t - sx sy'/T)/max(1, T-1);
 *   eigh(sym C0) with eigenvalues clipped at `clip` (the reference's NUMERIC_MIN_POSITIVE = 1e-12);
 *   S = C0^-1/2;  d_eigvals [F] = eigvalsh(sym(S Ct S')) in DESCENDING order (the caller takes the top n_out).
 * No host round trip.  F <= 256: one launch; 256 < F <= 2048: the same steps on the device-wide block Jacobi (see
 * msm_eigh); F > 2048: MSM_ERR_UNSUPPORTED. */
msm_status msm_onesided_tica_eigenvalues(msm_ctx* ctx, const double* d_moments, int F, double clip,
                                         double* d_eigvals);

/* The raw column sums msm_column_moments_partial would give ([cnt F][S1 F][S2 F] about d_shift, over every
 * frame of the segments) derived from the lagged moments of the SAME shift and segments plus the first
 * and last `lag` frames of each segment: 2 S1 = sx + sy + edges, 2 S2 = diag(M00) + edges^2.  Saves the
 * separate standardisation pass over X when the covariance pass runs anyway.  Finite data only (the
 * lagged moments impute NaN as 0 about the shift, which is the column mean only in the two-pass order);
 * at most 16 segments, lag >= 1.  Additive across shards like the inputs. */
msm_status msm_moments_from_lagged(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                                   const int64_t* h_seg_start, const int64_t* h_seg_stop, int n_seg, int lag,
                                   const double* d_shift, const double* d_moments, double* d_sums);

/* msm_moments_from_lagged and msm_standardise_params(d_sums, d_shift, F, n_rows, with_std, ...) in ONE launch of one
 * workgroup: d_sums as the former leaves them, d_mean / d_scale / d_inv_scale [F] as the latter, same bits.  For a
 * single shard (with several, the sums are all-reduced between the two).  d_zero_slot (8 bytes on the device, may be
 * NULL) is set to zero by the same launch: pointing it at the max |Y| word of a k-means fit state lets
 * msm_project_preset go without its clear. */
msm_status msm_moments_tail(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                            const int64_t* h_seg_start, const int64_t* h_seg_stop, int n_seg, int lag,
                            const double* d_shift, const double* d_moments, double* d_sums, double n_rows, int with_std,
                            double* d_mean, double* d_scale, double* d_inv_scale, double* d_zero_slot);

/* TICA solve on the device (deeptime 0.4.5 TICA._decomposition semantics):
 *   mean = (sx+sy)/(2T); C00 = M00/(2T) - mean mean'; C0t = (M0t+M0t')/(2T) - mean mean'
 *   (all divided by d_scale[i]*d_scale[j] when d_scale != NULL, i.e. covariances of
 *   the standardised data (x-shift)/scale);
 *   C00 = V S V' (Jacobi), keep |s| >= epsilon, canonical signs, L = V S^-1/2;
 *   eigh(L' C0t L), sort by descending magnitude, R = L R', canonical signs,
 *   kinetic_map != 0: column i of R scaled by eigenvalue i.
 * Outputs: d_eigvals [F] (0 beyond rank), d_coeffs [F, F] row-major with column i
 * = i-th TICA component (0 beyond rank), d_mean [F] = symmetric mean in
 * standardised coordinates, d_rank int32 [1].  No host sync.  F <= 256: one launch (a full-rank C00 is whitened by
 * a Cholesky / LDL' factor instead of the first eigensolve, which gives the same eigenpairs).  256 < F <= 2048: the steps
 * above, each spread over the device (block Jacobi eigensolves as in msm_eigh, multi-workgroup fp64 matrix-core
 * products); the rank stays in device memory.  F > 2048: MSM_ERR_UNSUPPORTED. */
msm_status msm_tica_solve(msm_ctx* ctx, const double* d_moments, const double* d_scale, int F,
                          double epsilon, int kinetic_map, double* d_eigvals, double* d_coeffs,
                          double* d_mean, int* d_rank);

/* The same solve when only the n_lead leading components are read (tica_reduce keeps `n_components` of them:
 * S/markov_state_model/reduction.py:109; deeptime 0.4.5 TICA(dim=...) truncates the same sorted list).
 * d_coeffs and d_eigvals are 0 from min(n_lead, rank) on; d_mean and d_rank as msm_tica_solve gives them.
 * n_lead <= 0 or n_lead >= F: msm_tica_solve.
 * F <= 64 (C00 of full rank or not), 2 (n_lead + 2) < rank: of the whitened rank x rank problem only the
 * n_lead + 2 eigenvalues at either end of the spectrum are bracketed and only the vectors of the n_lead + 1 at
 * either end are formed and tested.  Column i < n_lead of d_coeffs and d_eigvals[i] then carry the bits
 * msm_tica_solve gives them, with ONE exception: msm_tica_solve gives up the tridiagonal solver's result for Jacobi
 * when any of its rank vectors fails the residual or orthogonality test; a failure that involves a vector this
 * entry does not form goes unseen here, the tridiagonal result is kept, and the kept pairs agree with
 * msm_tica_solve to solver accuracy (the bounds both meet), not bit for bit.
 * Every other case (F > 64 -- orders above 256 included --, the Jacobi paths, 2 (n_lead + 2) >= rank, a tie in |eigenvalue| at the cut, an
 * eigenvalue within 1e-6 of the norm of the vectors formed) computes all pairs and truncates: bits always equal. */
msm_status msm_tica_solve_leading(msm_ctx* ctx, const double* d_moments, const double* d_scale, int F,
                                  double epsilon, int kinetic_map, double* d_eigvals, double* d_coeffs,
                                  double* d_mean, int* d_rank, int n_lead);

/* Y[t][c] = sum_f (((x[t][f] - mu[f]) * inv_sigma[f]) - mean2[f]) * W[f][c], fp64 FMA chain
 * over ascending f.  Replaces model.transform(X_prep) of tica_reduce
 * (S/markov_state_model/reduction.py:109).  NaN -> 0 after centring.
 * d_mean2 may be NULL.  W is [F, ldw] (first d columns used), Y is [n, ldy] f64.
 * d_absmax (f64 [1], may be NULL) receives max |Y| from the same pass: pointing it at slot 2 of a
 * k-means fit state and calling msm_kmeans_fit_begin with absmax_ready = 1 saves that call's own
 * pass over Y. */
msm_status msm_project(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                       const double* d_mu, const double* d_inv_sigma, const double* d_mean2,
                       const double* d_w, int d, int64_t ldw, double* d_y, int64_t ldy, double* d_absmax);

/* The same projection for X known to hold no NaN (msm_column_moments' d_count tells): the NaN test per element is
 * left out, same results on finite data.  With NaNs present the plain entry must be used. */
msm_status msm_project_finite(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                              const double* d_mu, const double* d_inv_sigma, const double* d_mean2,
                              const double* d_w, int d, int64_t ldw, double* d_y, int64_t ldy, double* d_absmax);

/* msm_project (assume_finite == 0) or msm_project_finite (!= 0) for a d_absmax word that an earlier call on the
 * same stream has already set to zero (msm_moments_tail's d_zero_slot): no clear of its own in front of the kernel.
 * A word that is not zero gives max(word, max |Y|). */
msm_status msm_project_preset(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                              const double* d_mu, const double* d_inv_sigma, const double* d_mean2,
                              const double* d_w, int d, int64_t ldw, double* d_y, int64_t ldy, double* d_absmax,
                              int assume_finite);

/* Symmetric eigendecomposition by parallel cyclic Jacobi, ascending
 * eigenvalues d_w [n], eigenvectors in the columns of d_v [n, n] (may be NULL).
 * Only the symmetric part of d_a is used.  n <= 256: one workgroup, one launch.  256 < n <= 2048: block Jacobi over
 * the whole device (blocks of 32, 2 + 3 (ceil(n / 32) - 1) stream-ordered launches per sweep, convergence flag in
 * device memory, no host sync; same results bit for bit on every call).  n > 2048: MSM_ERR_UNSUPPORTED.
 * d_sweeps reports the sweeps taken (40: the iteration ran out).
 * Replaces np.linalg.eigh on the path (e.g. _estimate_top_eigenvalues,
 * S/features/deeptica/core/trainer_api.py:646-651). d_sweeps int32 [1] may be NULL. */
msm_status msm_eigh(msm_ctx* ctx, const double* d_a, int n, double* d_w, double* d_v, int* d_sweeps);

/* Per-segment autocorrelation of the standardised columns at n_lag lags: the frame passes of
 * _autocorrelation_curve (S/analysis/diagnostics.py:247-351), which walks the split once per segment and lag.
 * For segment s = rows [start, stop) of length L, in fp64 whatever the input type:
 *   mean_f = column mean over the segment, var_f = mean of (x - mean_f)^2 (ddof = 0);
 *   column f is valid when var_f > var_floor (the reference passes 1e-8, an absolute number; a column that
 *   holds a non-finite value has a NaN variance and is not valid); d_nvalid[s] = m = number of valid columns;
 *   z = (x - mean_f) / sqrt(var_f) on the valid columns;
 *   d_value[s][l] = sum_{valid f} sum_{t = start}^{stop - tau - 1} z[t][f] z[t + tau][f] / ((L - tau) m)
 *   for 1 <= tau = h_lags[l] < L, and NaN when tau >= L, L <= 1 or m = 0.  Pairs never cross a segment.
 * The weighting of the segments into one curve is left to the host (pmarlo_amd/analysis/diagnostics.py).
 * Means and variances are formed first and the products from centred values, so a large common offset
 * costs no digits.  Per-workgroup partial sums go through a slab and are added in a fixed order: two calls
 * on the same input give the same bits.  The segments and lags travel through the context's device table,
 * any number of each; the launch sequence has 4 + 2 ceil(n_lag / 32) kernels whatever n_seg is.
 *
 * d_x [n, ld] f32 / f64, 1 <= F <= 256 (MSM_ERR_UNSUPPORTED beyond), ld >= F, n <= 2^31.
 * h_seg_start / h_seg_stop int64 [n_seg], n_seg >= 1, 0 <= start <= stop <= n (not clipped: anything else is
 * MSM_ERR_INVALID); h_lags int32 [n_lag], every lag >= 1.
 * d_value f64 [n_seg][n_lag] OVERWRITTEN; d_nvalid int32 [n_seg] OVERWRITTEN (may be NULL).
 * Not under graph capture. */
msm_status msm_autocorr_lagscan(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                                const int64_t* h_seg_start, const int64_t* h_seg_stop, int n_seg,
                                const int32_t* h_lags, int n_lag, double var_floor, double* d_value,
                                int32_t* d_nvalid);

/* d_out [n, pa + pb] f64 = [A | B]: the two column blocks side by side, so that ONE msm_lagged_moments(lag = 0)
 * pass over d_out gives the joint second moments the canonical correlations are made of
 * (_canonical_correlations, S/analysis/diagnostics.py:173-221).  A is [n, lda], B is [n, ldb], f32 or f64 each. */
msm_status msm_hstack_f64(msm_ctx* ctx, const void* d_a, msm_dtype dtype_a, int pa, int64_t lda, const void* d_b,
                          msm_dtype dtype_b, int pb, int64_t ldb, int64_t n, double* d_out);

/* Forward pass of a trained DeepTICA network in evaluation mode, all frames in one launch: what
 * DeepTICAModel.transform does before the output whitening (S/features/deeptica/_full.py:283-292), for the network
 * that override_core_mlp and PrePostWrapper build (S/features/deeptica/core/model.py:72-107, 355-368).
 *   Z = (x - mean) / scale in fp64 (sklearn's StandardScaler), ROUNDED TO FP32 as the reference's
 *       torch.as_tensor(Z, dtype=float32) does (_full.py:289); d_mean = d_scale = NULL: Z = x rounded to fp32;
 *   ln_in: LayerNorm over the F entries of the row (model.py:360; eps 1e-5, biased variance, affine);
 *   for each of the n_linear Linear layers of widths h_widths[0] = F, ..., h_widths[n_linear] = n_out:
 *       x <- x W' + b with W [out, in]; then, unless it is the last one, LayerNorm(out) when ln_hidden, and the
 *       activation (model.py:95-103); after the last one the activation when head_activation is set
 *       (model.py:104-105: linear_head false).  Dropout is the identity in evaluation.
 *   activation (resolve_activation_module, model.py:36-50): 0 tanh, 1 gelu (exact, erf), 2 relu, 3 elu (alpha 1),
 *       4 selu, 5 leaky_relu (slope 0.01).
 * The parameters are the fp32 values of the bundle, widened exactly; every product (v_mfma_f64_16x16x4_f64), sum,
 * LayerNorm (two-pass) and activation is fp64.  d_params, n_params floats, packed in this order:
 *   [gamma [F], beta [F]] of the input LayerNorm if ln_in;
 *   then for each Linear: W [out, in] row-major, b [out], and [gamma [out], beta [out]] if ln_hidden and it is not
 *   the last Linear.
 * n_params must equal what the widths need (MSM_ERR_INVALID otherwise).
 * A frame's outputs depend on that frame alone: the same bits whatever n is and wherever the frame sits.  A frame
 * with a non-finite Z (a NaN or Inf input, or one that overflows fp32) gets NaN in all its outputs.
 * d_x [n, ld] f32 / f64, ld >= F; d_out [n, ldo] f64, ldo >= n_out, columns from n_out on untouched.
 * Every width <= 256, n_out <= 64, 1 <= n_linear <= 8: MSM_ERR_UNSUPPORTED beyond, naming the number.
 * One plain launch on the context's stream, capturable. */
msm_status msm_mlp_forward(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                           const double* d_mean, const double* d_scale, int n_linear, const int32_t* h_widths,
                           int activation, int ln_in, int ln_hidden, int head_activation, const float* d_params,
                           size_t n_params, double* d_out, int64_t ldo);

/* ---- DeepTICA training: one step of the reference's curriculum trainer (S/ml/deeptica/trainer.py:1020-1070) ----
 *
 * VAMP-2 loss of VAMP2Loss.forward (S/features/deeptica/losses.py) with uniform weights 1/m, the case the reference's
 * trainer uses (per-pair weights: msm_vamp2_loss_weighted below), and its closed-form gradient with respect to the
 * outputs.  d_y0, d_yt [m, ld] f64: the network's outputs at the t and the tau frames, n_out <= 64 columns each.
 *   C00, Ctt, C0t: centred covariances of the outputs, correction 0;
 *   A = sym((1 - alpha) C00 + (alpha mu + max(mu eps, mu eps_abs)) I), mu = max(tr C00, 1e-12) / n_out; B likewise
 *       from Ctt; alpha is clamped to [0, 1], eps_abs and cond_reg to >= 0;
 *   cond A = max(l_max, 1e-12) / max(l_min, 1e-12) from the spectrum of A (cyclic Jacobi);
 *   A = L_A L_A' by Cholesky with the reference's jitter ladder (A + total I; total 0, then 1e-8, growth 10, five
 *       tries); score = |L_A^-1 C0t L_B^-T|_F^2; penalty = cond_reg (log max(1, cond A) + log max(1, cond B));
 *       loss = -score + penalty.
 * Gradient, with Ai, Bi the inverses of the factorised A, B and C = C0t:
 *   G_A = Ai C Bi C' Ai + cond_reg (v_max v_max' / l_max - v_min v_min' / l_min), G_B likewise, G_0t = -2 Ai C Bi,
 *   G_00 = (1 - alpha) G_A + (c / n_out) tr(G_A) I, c = alpha + max(eps, eps_abs); G_tt likewise;
 *   dloss/dZ0 = (2 Y0 G_00 + Yt G_0t') / m, dloss/dZt = (2 Yt G_tt + Y0 G_0t) / m with centred Y0, Yt.
 *   The penalty's part is absent when cond <= 1 (n_out = 1, and the clamp at 1) and, per eigenvalue, on the 1e-12
 *   floor; the trace part is absent when the trace sits on its floor.
 * d_stats [MSM_VAMP2_STATS] f64: [0] loss, [1] score, [2] penalty, [3] cond_C00, [4] cond_Ctt, [5] eig_C00_min,
 *   [6] eig_C00_max, [7] eig_Ctt_min, [8] eig_Ctt_max, [9] 1 when a Cholesky factorisation failed after the five
 *   tries (the reference raises; loss and score are then NaN), [10..15] zero; then var_z0, var_zt, mean_z0, mean_zt,
 *   64 entries each, the first n_out of each written.
 * d_grad0, d_gradt [m, ldg] f64 or both NULL.  d_work: msm_vamp2_workspace(m, n_out) bytes (0: outside the
 * envelope).  Envelope: 1 <= m <= 2^24 (the moments kernels take one chunk per grid row and the device admits 65536
 * rows) and n_out <= 64; MSM_ERR_UNSUPPORTED beyond, naming the number, before anything is launched.  Moments are summed per chunk of 256 frames on the matrix cores and the chunks added in ascending
 * order, the dense algebra runs in one workgroup: equal inputs give equal bits.  Plain launches on the context's
 * stream, no host synchronisation. */
#define MSM_VAMP2_STATS 272
size_t msm_vamp2_workspace(int64_t m, int n_out);
msm_status msm_vamp2_loss(msm_ctx* ctx, const double* d_y0, const double* d_yt, int64_t m, int n_out, int64_t ld,
                          double eps, double eps_abs, double alpha, double cond_reg, double* d_work,
                          double* d_stats, double* d_grad0, double* d_gradt, int64_t ldg);

/* Loss and parameter gradient of one batch of lagged pairs.  The network, its packed parameters and the scaler
 * are msm_mlp_forward's; d_x [n, ld] is the resident frame array, and the batch is 2m slots: slot s < m is row
 * d_idx_t[s], slot m + s is row d_idx_tau[s] (int64; a row outside [0, n) is not read and makes the loss NaN).
 * Training mode (model.py:72-107, 355-368): Z, input LayerNorm, input dropout; per Linear: Linear, LayerNorm,
 * activation, hidden dropout; the head gets the activation when head_activation is set and no dropout.
 * Everything after the fp32 rounding of Z is fp64.
 * Dropout: h_dropout [n_linear] (host): probability of site 0 (the inputs) and of site i (after the activation of
 *   Linear i - 1); NULL: evaluation mode.  0 <= p < 1, MSM_ERR_INVALID otherwise.  An element (site, slot, column) is
 *   kept iff word (column & 3) of Philox4x32-10 with key = seed and counter = {step, site, slot, column >> 2} is
 *   >= floor(p 2^32); every element is multiplied by 1 / (1 - p) if kept and by 0 otherwise, in fp64.  step < 2^32.
 *   The stream is not torch's.
 * With dropout off the outputs are bit-identical to msm_mlp_forward on the gathered rows.
 * d_stats as msm_vamp2_loss.  d_grad [n_params] f64 or NULL (no backward pass): dloss/dparameter in the packed
 * order, by the usual adjoints.  d_out [2m, ldo] f64 or NULL: the outputs by slot.  d_work: at least
 * msm_mlp_train_workspace(...) bytes (0: outside the envelope), given in work_bytes.
 * Parameter gradients are summed over the slots per chunk of 256 on the matrix cores, the chunks added in
 * ascending order; no floating-point atomics: equal inputs give equal bits.
 * Envelope: msm_mlp_forward's, and 2 <= m <= 2^24; MSM_ERR_UNSUPPORTED beyond, naming the number. */
size_t msm_mlp_train_workspace(int64_t m, int n_linear, const int32_t* h_widths, int ln_in, int ln_hidden,
                               int head_activation);
msm_status msm_mlp_loss_grad(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                             const double* d_mean, const double* d_scale, int n_linear, const int32_t* h_widths,
                             int activation, int ln_in, int ln_hidden, int head_activation, const float* d_params,
                             size_t n_params, const int64_t* d_idx_t, const int64_t* d_idx_tau, int64_t m,
                             const double* h_dropout, uint64_t seed, uint64_t step, double eps, double eps_abs,
                             double alpha, double cond_reg, double* d_work, size_t work_bytes, double* d_stats,
                             double* d_grad, double* d_out, int64_t ldo);

/* The same loss under per-pair weights (VAMP2Loss.forward(z0, zt, weights), losses.py:58-77).  d_w [m] f64:
 *   w'_s = max(w_s, 0); W = sum w'_s; what_s = w'_s / W;
 *   mu0 = sum what_s y0_s, mut likewise; C00 = sum what_s (y0_s - mu0)(y0_s - mu0)', Ctt, C0t likewise;
 *   from there the law above, unchanged (the same solve kernel, dividing by W where it divides by m);
 *   dloss/dZ0_s = what_s (2 (y0_s - mu0) G_00 + (yt_s - mut) G_0t'), dloss/dZt_s = what_s (2 (yt_s - mut) G_tt +
 *   (y0_s - mu0) G_0t): the weighted means add nothing, the weighted centred sums being zero.
 * Only the ratios of the weights matter.  The closed form is that of autograd wherever at least n_out + 2 pairs
 * carry positive weight (with fewer the smallest eigenvalue is tied and the penalty has no direction).
 * Divergence from the reference: W must be positive and finite, and every weight finite.  Otherwise loss, score and
 * all else are NaN and d_stats[10] = 1; no gradient is promised.  (The reference clamps W at 1e-12 and torch's cov
 * then raises "weights sum to zero".)
 * d_stats as msm_vamp2_loss, and [11] = W, [12] = W^2 / sum w'^2 (Kish's effective number of pairs).
 * Kernels: per chunk of 256 pairs the sums of w', w'^2, w' y0 and w' yt; the weighted centred second moments on the
 * matrix cores, one operand carrying w'_s; the solve; the weighted output gradient.  Chunks are added in ascending
 * order, no floating-point atomics: equal inputs give equal bits.  A weight past pair m is never read.
 * d_work: msm_vamp2_weighted_workspace(m, n_out) bytes.  Envelope, NULL and stride checks: msm_vamp2_loss's. */
size_t msm_vamp2_weighted_workspace(int64_t m, int n_out);
msm_status msm_vamp2_loss_weighted(msm_ctx* ctx, const double* d_y0, const double* d_yt, const double* d_w, int64_t m,
                                   int n_out, int64_t ld, double eps, double eps_abs, double alpha, double cond_reg,
                                   double* d_work, double* d_stats, double* d_grad0, double* d_gradt, int64_t ldg);

/* msm_mlp_loss_grad with the weighted loss: d_w [m] f64 is the weight of pair s (slots s and m + s).  Forward pass,
 * backward pass and parameter contractions are msm_mlp_loss_grad's own kernels; they receive the weighted dL/dY.
 * d_w NULL is msm_mlp_loss_grad itself (its workspace, its bits).  d_work: at least
 * msm_mlp_train_weighted_workspace(...) bytes; messages name msm_mlp_loss_grad. */
size_t msm_mlp_train_weighted_workspace(int64_t m, int n_linear, const int32_t* h_widths, int ln_in, int ln_hidden,
                                        int head_activation);
msm_status msm_mlp_loss_grad_weighted(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                                      const double* d_mean, const double* d_scale, int n_linear,
                                      const int32_t* h_widths, int activation, int ln_in, int ln_hidden,
                                      int head_activation, const float* d_params, size_t n_params,
                                      const int64_t* d_idx_t, const int64_t* d_idx_tau, const double* d_w, int64_t m,
                                      const double* h_dropout, uint64_t seed, uint64_t step, double eps, double eps_abs,
                                      double alpha, double cond_reg, double* d_work, size_t work_bytes, double* d_stats,
                                      double* d_grad, double* d_out, int64_t ldo);

/* The launch shape of the four per-frame network kernels, as the one host function all four launch sites call
 * decides it on this context now.  Launches nothing (above 48 KiB of LDS it raises the kernel's dynamic LDS limit,
 * as a launch would).
 *   kernel: MSM_MLP_KERNEL_FORWARD (msm_mlp_forward), _VJP (msm_mlp_vjp), _TRAIN_FORWARD, _TRAIN_BACKWARD (the two
 *       passes of msm_mlp_loss_grad); dtype: that of d_x (the backward pass has one instance, dtype is only checked);
 *   rows: n, or the 2m slots of a training batch (even, 2 <= m <= 2^24).
 * A workgroup is one wave that takes a group of 16 rows at a time; one round of workgroups is launched, as many as
 * are resident at once, and a workgroup that is given more than one group reuses its two LDS images.
 * out: [0] LDS bytes per workgroup, [1] workgroups resident per CU, [2] grid = min(groups, CUs x [1]),
 *   [3] groups = ceil(rows / 16), [4] trips = ceil(groups / grid) (0 when rows = 0); for the training kernels also
 *   [5] chunks of the parameter gradient = ceil(2m / MSM_MLP_CHUNK), [6] chunks of the loss's moments =
 *   ceil(m / MSM_MLP_CHUNK), [7] jobs of the parameter kernel (its grid is [7] x [5]); otherwise zero.
 * Envelope and codes: msm_mlp_forward's for the widths, msm_mlp_loss_grad's for m. */
#define MSM_MLP_CHUNK 256 /* slots (pairs) per partial sum of a parameter gradient (of a loss moment) */
#define MSM_MLP_KERNEL_FORWARD 0
#define MSM_MLP_KERNEL_VJP 1
#define MSM_MLP_KERNEL_TRAIN_FORWARD 2
#define MSM_MLP_KERNEL_TRAIN_BACKWARD 3
msm_status msm_mlp_launch_plan(msm_ctx* ctx, int kernel, msm_dtype dtype, int64_t rows, int n_linear,
                               const int32_t* h_widths, int ln_in, int ln_hidden, int head_activation, int64_t out[8]);

/* Gradient clip (trainer.py:1048-1060, torch's clip_grad_norm_) and one step of torch's AdamW with a single
 * parameter group, all in fp64:
 *   norm = |g|_2; clip > 0: g <- g min(1, clip / (norm + 1e-6)); clip <= 0: none;
 *   p <- p (1 - lr wd); m <- beta1 m + (1 - beta1) g; v <- beta2 v + (1 - beta2) g^2;
 *   p <- p - (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps); step counts from 1.
 * d_params [n] f32 is rounded once; d_m, d_v [n] f64.  d_out [4] f64: norm, norm after the clip, 1 when the norm
 * is not finite, the clip coefficient.  Divergence from the reference: a non-finite norm skips the update (p, m, v
 * untouched) and raises the flag; the reference would poison the parameters. */
msm_status msm_adamw_step(msm_ctx* ctx, float* d_params, const double* d_grad, double* d_m, double* d_v, int64_t n,
                          int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                          double clip, double* d_out);

/* ---- Using a trained network: the gradient with respect to the inputs, and the bias potential -------------------
 *
 * msm_mlp_vjp: forward pass in evaluation mode and the vector-Jacobian product with respect to the input rows, for
 * the network, packed parameters and scaler of msm_mlp_forward, in ONE launch (forward and backward of a group of 16
 * frames back to back, the tape read while it is still in L2).
 *   d_out [n, ldo] f64 or NULL: the outputs, bit-identical to msm_mlp_forward's.
 *   d_energy [n] f64 or NULL: strength * sum_c y_c^2.
 *   d_gout [n, ldgo] f64: the upstream gradient dE/dy; NULL: E is the energy above and 2 strength y goes upstream.
 *   d_gx [n, ldgx] f64, ldgx >= F: dE/dx.  The adjoints are those of msm_mlp_loss_grad with dropout off, carried on
 *       past the first Linear (dA_0 = du_0 W_0), through the input LayerNorm if there is one, to dx = dZ / scale;
 *       the fp32 rounding of Z is the identity for the derivative (as .to(float32) is in torch).  All fp64.
 *   d_work: msm_mlp_vjp_workspace(...) bytes (0: outside the envelope), given in work_bytes: per frame the scaled
 *       inputs (with an input LayerNorm), each hidden LayerNorm's input and each activation's argument.
 * A frame with a non-finite Z is NaN in its own rows of d_out, d_energy and d_gx only; every result of a frame
 * depends on that frame alone, bit for bit.  Envelope and messages are msm_mlp_forward's.  Capturable.
 *
 * msm_bias_energy_forces: the harmonic bias of a DeepTICA collective variable (CVBiasPotential with
 * HarmonicExpansionBias, S/features/deeptica/cv_bias_potential.py): positions and box -> features
 * (msm_featurize_spec) -> scaler and network -> E = strength * sum cv^2, and the force -dE/dx on every atom.
 *   Three plain launches on the context's stream -- msm_featurize_spec, msm_mlp_vjp with d_gout = NULL,
 *   msm_featurize_spec_vjp with sign = -1 -- no host synchronisation, capturable; n = 1 is one MD step.  The
 *   features are msm_featurize_spec's bits, except that a record reading a non-finite coordinate gives NaN (in that
 *   function a dihedral or a contact of a NaN coordinate is 0 and a lone infinite coordinate is a +inf distance).
 *   The table has n_rec records and its width is the network's F = h_widths[0]; every column in [0, F) must be
 *   written by a record (a column no record writes would be read uninitialised).  d_inc_ptr / d_inc: the table's
 *   incidence (msm_featurize_spec_vjp).  d_energy [n], d_cv [n, ldo] or NULL (the raw network outputs), d_force
 *   [n, A, 3], all f64.  d_work: msm_bias_workspace(...) bytes: features f32 [n, F], their gradient f64 [n, F] and
 *   msm_mlp_vjp's tape.  Whatever one of the three steps would refuse is refused before the first launches.
 *   A frame with a NaN coordinate, an invalid record or (with flagged records) a singular box has NaN energy, CVs
 *   and forces; no other frame is disturbed. */
size_t msm_mlp_vjp_workspace(int64_t n, int n_linear, const int32_t* h_widths, int ln_in, int ln_hidden,
                             int head_activation);
msm_status msm_mlp_vjp(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                       const double* d_mean, const double* d_scale, int n_linear, const int32_t* h_widths,
                       int activation, int ln_in, int ln_hidden, int head_activation, const float* d_params,
                       size_t n_params, const double* d_gout, int64_t ldgo, double strength, double* d_energy,
                       double* d_out, int64_t ldo, double* d_gx, int64_t ldgx, double* d_work, size_t work_bytes);
size_t msm_bias_workspace(int64_t n, int F, int n_linear, const int32_t* h_widths, int ln_in, int ln_hidden,
                          int head_activation);
msm_status msm_bias_energy_forces(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const float* d_box,
                                  int64_t n_box, const int32_t* d_rec, const float* d_param, int n_rec,
                                  const int32_t* d_inc_ptr, const int32_t* d_inc, int mic, const double* d_mean,
                                  const double* d_scale, int n_linear, const int32_t* h_widths, int activation,
                                  int ln_in, int ln_hidden, int head_activation, const float* d_params,
                                  size_t n_params, double strength, double* d_work, size_t work_bytes,
                                  double* d_energy, double* d_cv, int64_t ldo, double* d_force);

/* ------------------------------------------------------------------ */
/* k-means                                                          */
/* ------------------------------------------------------------------ */

/* Assign every frame to its nearest centre.
 * Replaces _KMeansDiscretizer.transform (S/analysis/discretize.py:471-494:
 * whiten with (x-mean)/std_safe, then sklearn predict) and the deeptime
 * model.transform of cluster_microstates (S/markov_state_model/
 * clustering.py:608-609).
 *
 *   z      = d_mean ? (x - mean[f]) / std[f] : x        (fp64, IEEE division)
 *   dot_j  = fma chain over f = 0..d-1 of z[f]*c[j][f], starting from +0.0
 *   dist_j = fma(-2.0, dot_j, |c_j|^2)      |c_j|^2 = fma chain of c[j][f]^2
 *   label  = first j with minimal dist_j (strict <, ties -> lowest index)
 *
 * which is sklearn's argmin_j(|c_j|^2 - 2 x.c_j) (lloyd_iter_chunked_dense)
 * with the summation order pinned; oracle/msm_oracle.c restates it with C fma().
 *
 * d_x  [n, ld] dtype   d_centers f64 [k, d]   d_mean/d_std f64 [d] or NULL   (1 <= d <= 256;
 * wider frames return MSM_ERR_UNSUPPORTED)
 * d_labels int32 [n]   d_mindist f64 [n] or NULL (dist_j + |z|^2 >= 0 clipped,
 * i.e. the squared distance to the chosen centre, for inertia)
 */
msm_status msm_kmeans_assign(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d,
                             int64_t ld, const double* d_centers, int k,
                             const double* d_mean, const double* d_std,
                             int32_t* d_labels, double* d_mindist);

/* ---- k-means fit (Lloyd) ------------------------------------------------
 * Replaces the estimator.fit of _KMeansDiscretizer.fit (S/analysis/discretize.py:
 * 458-469, sklearn KMeans / MiniBatchKMeans) and of cluster_microstates
 * (S/markov_state_model/clustering.py:605-609, deeptime KMeans.fit_fetch).
 * Bit-level parity with those RNG-driven fits is not attainable (SURVEY.md hard
 * part 2): the contract is (a) assignment parity given identical centres
 * (msm_kmeans_assign), (b) inertia no worse than the reference's, (c) run-to-run
 * and shard-count independence of the result for a fixed seed.
 *
 * Initial centres: k frames drawn by stratified sampling along the time axis
 * (frame floor((j + u_j) n / k), u_j = splitmix64(seed, j)), whitened like the data.
 * Iteration: assign (same arithmetic as msm_kmeans_assign) + accumulate member sums
 * in 64-bit fixed point (integer atomics: order independent, exact across shards),
 * then centres = sums / counts; empty clusters keep their centre.
 *
 * d_state: 8 doubles on the device = {scale, inv_scale, absmax, shift2, tol2, done,
 * n_iter, inertia}.  Iterations after convergence (shift2 <= tol2) are no-ops, so a
 * fixed launch sequence (or a captured graph) needs no host round trip.
 *
 * msm_kmeans_fit        = begin + max_iter x (accumulate + update) on one device.
 * msm_kmeans_fit_begin  computes the fixed-point scale from max|z| and n_total (the
 *                       frame count over ALL shards) and, if init_centers != 0, the
 *                       initial centres.  Shards then all-reduce MIN of state[0].
 *                       absmax_ready != 0: state[2] already holds max|x| (msm_project's d_absmax);
 *                       only without whitening (d_mean == NULL).
 * msm_kmeans_accumulate adds this shard's member sums / counts into d_sums int64 [k*d],
 *                       d_counts int64 [k] (caller zeroes them; all-reduce SUM across shards).
 * msm_kmeans_update     centres <- sums/counts, shift2, done, n_iter; clear != 0 zeroes
 *                       the accumulators for the next iteration. */
msm_status msm_kmeans_fit(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d, int64_t ld,
                          const double* d_mean, const double* d_std, int k, uint64_t seed,
                          int init_centers, int max_iter, double tol2, double* d_centers,
                          double* d_state);
/* k-means++ seeding (deeptime KMeans init_strategy = 'kmeans++', S/markov_state_model/clustering.py:322-361;
 * sklearn KMeans init = 'k-means++', S/analysis/discretize.py:458-469): after msm_kmeans_fit_begin (which leaves
 * max |z| in d_state[2]) this replaces the k centres by frames drawn with probability proportional to the squared
 * distance to the nearest centre already drawn.  Integer weights and splitmix64 draws (csrc/kmeanspp.hip): the
 * frames drawn are a function of the data and the seed alone, and oracle/npport.kmeans_plusplus repeats them bit
 * for bit.  d_picked (int64 [k], may be NULL) receives the frame numbers.  The weights are summed per block of
 * MSM_KPP_BLOCK frames; the one workgroup that draws gives each of its MSM_KPP_BLOCK threads
 * ceil(blocks / MSM_KPP_BLOCK) consecutive block sums. */
#define MSM_KPP_BLOCK 1024
msm_status msm_kmeans_init_plusplus(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d, int64_t ld,
                                    const double* d_mean, const double* d_std, int k, uint64_t seed, double n_total,
                                    double* d_centers, const double* d_state, int64_t* d_picked);
msm_status msm_kmeans_fit_begin(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d,
                                int64_t ld, const double* d_mean, const double* d_std, int k,
                                uint64_t seed, int init_centers, double n_total, double tol2,
                                double* d_centers, double* d_state, int absmax_ready);
/* msm_kmeans_fit_begin that also zeroes the member sums of the fit that begins (d_sums int64 [k*d], d_counts int64
 * [k]): by the launch that draws the centres (init_centers != 0), so the caller's clear of them falls away. */
msm_status msm_kmeans_fit_begin_clear(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d,
                                      int64_t ld, const double* d_mean, const double* d_std, int k,
                                      uint64_t seed, int init_centers, double n_total, double tol2,
                                      double* d_centers, double* d_state, int absmax_ready, int64_t* d_sums,
                                      int64_t* d_counts);
msm_status msm_kmeans_accumulate(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d,
                                 int64_t ld, const double* d_centers, int k, const double* d_mean,
                                 const double* d_std, const double* d_state, int64_t* d_sums,
                                 int64_t* d_counts);
msm_status msm_kmeans_update(msm_ctx* ctx, int64_t* d_sums, int64_t* d_counts, int k, int d,
                             double* d_centers, double* d_state, int clear);

/* Frame images for the certified fp16 filter (pmarlo_amd/csrc/kmeans_filter.h).  For d <= 10 and a centre
 * table that fits the LDS (k <= ~750 at d = 10) msm_kmeans_assign / _accumulate / _fit take the labels from an
 * fp16 matrix-core pass over two-way fp16 splits of the power-of-two scaled coordinates: an upper bound of every pinned fp64 score,
 * the winner's candidates re-scored with the pinned fp64 chain and accepted only when they beat every bound
 * outside the candidate set; the remaining ~1 % of the frames take an exhaustive fp64 scan.  Labels, ties,
 * distances and member sums are those of the all-fp64 arithmetic stated at msm_kmeans_assign, bit for bit
 * (same reference lines: S/analysis/discretize.py:471-494, S/markov_state_model/clustering.py:608-609).
 *
 * The image of a frame (its split coordinates in matrix-operand order, 48 bytes) depends only on the
 * frame, the whitening and the shard's scale, so a caller that runs many passes over the same frames (Lloyd iterations) builds
 * it once with msm_kmeans_pack and hands it to the _packed entry points; the plain entry points build it per
 * call in a buffer of the context.  d_image == NULL or a shape outside the filter's range: same as the plain
 * call.  msm_kmeans_image_bytes gives the size (0 for d > 10); the buffer must be 16-byte aligned.
 * msm_kmeans_filter_scanned reports (and optionally clears) the number of frames that took the exhaustive
 * scan since the context was created: diagnostics only. */
msm_status msm_kmeans_image_bytes(int64_t n, int d, size_t* out_bytes);
msm_status msm_kmeans_pack(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d, int64_t ld,
                           const double* d_mean, const double* d_std, void* d_image);
/* The same with d_absmax: a DEVICE pointer to one double >= max |x| over the frames (whitened when d_mean /
 * d_std are given; e.g. slot 2 of a k-means fit state), from which the frames' power-of-two scale follows;
 * msm_kmeans_pack finds it with a pass of its own. */
msm_status msm_kmeans_pack_bounded(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d, int64_t ld,
                                   const double* d_mean, const double* d_std, const double* d_absmax, void* d_image);
msm_status msm_kmeans_assign_packed(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d,
                                    int64_t ld, const double* d_centers, int k, const double* d_mean,
                                    const double* d_std, const void* d_image, int32_t* d_labels,
                                    double* d_mindist);
msm_status msm_kmeans_accumulate_packed(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d,
                                        int64_t ld, const double* d_centers, int k, const double* d_mean,
                                        const double* d_std, const void* d_image, const double* d_state,
                                        int64_t* d_sums, int64_t* d_counts);
/* Incremental form of the accumulate pass: d_prev_labels int32 [n] holds the centre each frame is booked under
 * (-1: none yet) and is updated in place; a frame whose centre did not change is left alone, one that moved is
 * subtracted from its old centre's sums / count and added to the new one's.  d_sums / d_counts must therefore
 * PERSIST between calls (msm_kmeans_update with clear = 0).  The sums are 64-bit fixed-point integers, so they hold
 * the bits of a full re-accumulation; after the first passes of a Lloyd run only a few per cent of the frames move.
 * d_image may be NULL. */
msm_status msm_kmeans_accumulate_delta(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d,
                                       int64_t ld, const double* d_centers, int k, const double* d_mean,
                                       const double* d_std, const void* d_image, const double* d_state,
                                       int32_t* d_prev_labels, int64_t* d_sums, int64_t* d_counts);
/* One whole Lloyd iteration: the accumulate pass above (incremental when d_prev_labels is given, which then needs
 * persistent d_sums / d_counts) followed by msm_kmeans_update(clear = 0) on d_centers / d_state -- in ONE launch where
 * the filter kernel runs: the workgroup that finishes last closes the iteration, with the bits of the separate update
 * kernel.  For a single shard; with several shards the sums are reduced between the two halves
 * (msm_kmeans_accumulate_delta, msm_allreduce_i64_from, msm_kmeans_update).
 * Reference: one iteration of deeptime KMeans.fit / sklearn KMeans behind cluster_microstates
 * (S/markov_state_model/clustering.py:322-361) and _KMeansDiscretizer.fit (S/analysis/discretize.py:458-469). */
msm_status msm_kmeans_lloyd_pass(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d, int64_t ld,
                                 double* d_centers, int k, const double* d_mean, const double* d_std,
                                 const void* d_image, double* d_state, int32_t* d_prev_labels, int64_t* d_sums,
                                 int64_t* d_counts);
/* The two incremental entry points with first_pass: != 0 on the first pass of a fit, when no frame is booked under a
 * centre yet.  d_prev_labels then need not hold -1: its contents are ignored (the filter kernel does not read them; for
 * shapes that run the all-fp64 kernel the call fills the buffer itself) and every frame is added to its centre, as
 * after a fill with -1.  first_pass == 0: the entry points above. */
msm_status msm_kmeans_accumulate_delta_from(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d,
                                            int64_t ld, const double* d_centers, int k, const double* d_mean,
                                            const double* d_std, const void* d_image, const double* d_state,
                                            int32_t* d_prev_labels, int64_t* d_sums, int64_t* d_counts,
                                            int first_pass);
msm_status msm_kmeans_lloyd_pass_from(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d, int64_t ld,
                                      double* d_centers, int k, const double* d_mean, const double* d_std,
                                      const void* d_image, double* d_state, int32_t* d_prev_labels, int64_t* d_sums,
                                      int64_t* d_counts, int first_pass);
/* The deferred chain: a second way of chaining the Lloyd passes of a single-shard fit, with the bits of
 * msm_kmeans_lloyd_pass_from + msm_kmeans_assign_packed after every launch.  A pass ends with the flush of its member
 * sums; the NEXT launch (a pass, or the closing assign) closes the iteration in its prologue: every workgroup computes
 * centres <- sums / counts for itself from what the kernel boundary has ordered, keeps them in its LDS, and one of them
 * writes d_centers_out and the fit state.  No workgroup waits for another inside a launch.
 *   d_centers_in   the centres before the pending close (read only); d_centers_out receives the centres the launch
 *                  works with (close_pending != 0: a different buffer; the caller alternates two)
 *   close_pending  0 on the first pass of a fit (nothing to close: d_centers_in are the centres, d_sums_in is not read)
 *   member sums    rotate through THREE buffers, so that no workgroup reads what another adds to in the same launch:
 *                  d_sums_in / d_counts_in hold the complete sums of the previous pass; d_sums_out / d_counts_out must be
 *                  ZERO when the launch begins and receive in + the moves of this pass; d_sums_next / d_counts_next are
 *                  cleared for the launch after this one.  (First pass: `out` cleared by msm_kmeans_fit_begin_clear.)
 *   a fit that has converged (state.done): later passes compute nothing and keep both rotations going.
 * Incremental only: d_prev_labels is required (first_pass as in msm_kmeans_lloyd_pass_from).
 * *h_applied (HOST int) = 1 when the launch was made, 0 (and MSM_OK, nothing launched or written) where this flavour
 * does not run -- fp32 frames, whitening, d <= 4 or d > 10, k d > 5120, no image, or the fp64 centre table does not fit
 * the LDS next to the rest: the caller then runs the entry points above.  msm_kmeans_assign_closing: the assignment
 * under the centres of the pending close (labels, d_mindist as msm_kmeans_assign); close_pending == 0: d_centers_in as
 * they are, d_state / sums may be NULL. */
msm_status msm_kmeans_lloyd_pass_deferred(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d, int64_t ld,
                                          const double* d_centers_in, double* d_centers_out, int k,
                                          const double* d_mean, const double* d_std, const void* d_image,
                                          double* d_state, int32_t* d_prev_labels, const int64_t* d_sums_in,
                                          const int64_t* d_counts_in, int64_t* d_sums_out, int64_t* d_counts_out,
                                          int64_t* d_sums_next, int64_t* d_counts_next, int close_pending,
                                          int first_pass, int* h_applied);
msm_status msm_kmeans_assign_closing(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int d, int64_t ld,
                                     const double* d_centers_in, double* d_centers_out, int k, const double* d_mean,
                                     const double* d_std, const void* d_image, double* d_state,
                                     const int64_t* d_sums_in, const int64_t* d_counts_in, int close_pending,
                                     int32_t* d_labels, double* d_mindist, int* h_applied);
msm_status msm_kmeans_filter_scanned(msm_ctx* ctx, uint64_t* h_out, int reset);
/* Hardware rule the filter's certificate rests on (kmeans_filter.h, step 1): n_tiles independent
 * v_mfma_f32_16x16x32_bf16 instructions, D = A B + C with A [16][32], B [32][16] bf16 (row major, raw 16-bit
 * patterns) and C, D [16][16] f32, all HOST arrays.  tests/test_gpu_mfma_rule.py checks the accumulation
 * bound, the irrelevance of the slot order and the treatment of small terms on every box the suite runs on. */
msm_status msm_mfma_bf16_probe(msm_ctx* ctx, const uint16_t* h_a, const uint16_t* h_b, const float* h_c,
                               float* h_d, int n_tiles);
/* The same with one v_mfma_f32_16x16x32_f16 per tile (A, B raw fp16 patterns): the instruction of the fp16
 * filter.  tests/test_gpu_mfma_rule_f16.py measures its accumulation bound and its treatment of subnormals. */
msm_status msm_mfma_f16_probe(msm_ctx* ctx, const uint16_t* h_a, const uint16_t* h_b, const float* h_c,
                              float* h_d, int n_tiles);

/* d_out[0] = sum of d_v[0..n) with a fixed-order two-level reduction (inertia =
 * sum of msm_kmeans_assign's d_mindist; clustering.py:391-392). */
msm_status msm_sum_f64(msm_ctx* ctx, const double* d_v, int64_t n, double* d_out);

/* ------------------------------------------------------------------ */
/* MSM estimation: transition matrix, stationary distribution, ITS      */
/* ------------------------------------------------------------------ */

/* Count matrix -> transition matrix.  d_counts is int64 [k*k] (counts_are_f64 = 0)
 * or float64 [k*k].  d_rowsum f64 [k] receives the row sums of the counts.
 *  mode 0: T = C / rowsum, all-zero rows stay zero, full k x k
 *          (_normalise_counts, S/analysis/discretize.py:678-682); d_diag_mass (may be
 *          NULL) = trace(T)/k (discretize.py:1059-1062).
 *  mode 1: ensure_connected_counts + MaximumLikelihoodMSM(reversible=False)
 *          (S/utils/msm_utils.py:129-167, S/markov_state_model/_estimation.py:158-188):
 *          active = states with rowsum + colsum > epsilon (ascending), C_active + alpha on
 *          every cell, T_active = row-normalised.  T_active is written PACKED into the
 *          top-left n_active x n_active corner of d_T with row stride k; d_active int32 [k]
 *          lists the active states, d_inv_map int32 [k] maps state -> packed index or -1,
 *          d_n_active int32 [1]. */
msm_status msm_transition_matrix(msm_ctx* ctx, const void* d_counts, int counts_are_f64, int k, int mode,
                                 double alpha, double epsilon, double* d_T, int32_t* d_active,
                                 int32_t* d_inv_map, int32_t* d_n_active, double* d_rowsum,
                                 double* d_diag_mass);

/* T_full = identity with the active block of a mode-1 result embedded, pi_full = 0
 * outside the active set (_estimation.py:174-181).  d_pi_active / d_pi_full may be NULL. */
msm_status msm_embed_full(msm_ctx* ctx, const double* d_T_active, const double* d_pi_active,
                          const int32_t* d_inv_map, int k, double* d_T_full, double* d_pi_full);

/* Leading spectrum of `batch` row-stochastic matrices (matrix b at d_T + b*t_stride, row
 * stride ld, order d_n[b] or n_max when d_n is NULL) by subspace iteration on T' with
 * Rayleigh-Ritz (one workgroup per matrix; the lag scan batches its lags).
 * Replaces deeptime stationary_distribution + eigenvalues(T, k) as used by
 * _finalize_transition_and_stationary and _summarize_its_stats
 * (S/markov_state_model/_its.py:543-604), and utils.safe_timescales (utils.py:17-57).
 *   p        subspace size (<= 32; use n_its + 1 + guard vectors)
 *   n_iter   iterations this call; init != 0 (re)starts from a seeded basis, init == 0
 *            continues from the basis left in d_workspace by the previous call
 *   d_ritz   f64 [batch][128] = {re[32] | im[32] | previous call's re[32] | im[32]},
 *            Ritz values sorted by descending magnitude (the caller keeps the buffer between calls)
 *   d_change f64 [batch]: convergence measure of the top n_watch Ritz values -- the residual
 *            ||T'x - theta x|| / ||x|| of every Ritz pair (complex pairs in real arithmetic through the
 *            real invariant plane; for them the smaller of the residual and the relative change of
 *            the value since the previous call counts) -- the caller relaunches with init = 0 until
 *            it is small
 *   d_pi     f64 [batch][pi_stride] stationary distribution (sum 1), or NULL
 *   n_its>0: d_its_eig / d_its_ts f64 [batch][n_its]: the top (n_its+1) values re-sorted by
 *            descending real part, first dropped, |real part| clipped to [1e-12, 1-1e-12],
 *            t = -max(1, lag)/ln(.), lag = d_lags[b]; NaN padding when fewer exist
 *   d_status int32 [batch]: 0, or the hqr failure index
 *   freeze_tol > 0 with init == 0: matrices whose d_change (left by the previous call) is already
 *            <= freeze_tol are skipped and keep all their outputs (uneven batches: lag scans,
 *            posterior samples); 0 iterates every matrix
 *   d_vecs   f64 [batch][n_vecs][n_max] or NULL: left eigenvectors (x'T = theta x') of the Ritz values
 *            in descending magnitude, unit 2-norm, largest-magnitude component positive; NaN rows for
 *            complex pairs.
 *            For a reversible T the right eigenvectors are x / pi (PCCA+ input)
 * d_workspace must hold msm_spectrum_workspace_bytes(n_max, p, batch) bytes. */
size_t msm_spectrum_workspace_bytes(int n_max, int p, int batch);
msm_status msm_spectrum(msm_ctx* ctx, const double* d_T, int64_t t_stride, int ld, const int32_t* d_n,
                        int n_max, int batch, int p, int n_iter, int init, uint64_t seed, int n_watch,
                        void* d_workspace, double* d_ritz, double* d_pi, int64_t pi_stride,
                        double* d_change, int32_t* d_status, int n_its, const double* d_lags,
                        double* d_its_eig, double* d_its_ts, double freeze_tol, double* d_vecs, int n_vecs);
/* d_out <- T^(2^n_squarings) for the same batch layout (fp64 matrix cores; entries outside the d_n[b] x d_n[b] block
 * zero).  d_scratch: a second buffer of the batch's size (may be NULL for one squaring).  msm_spectrum_powered is
 * msm_spectrum with the ITERATIONS run on such a power d_T_power (same invariant subspaces, the convergence ratio
 * raised to that power: a quarter of the iterations with T^4); the Rayleigh-Ritz values, residuals, pi, implied
 * timescales and vectors are those of d_T itself.  Same reference operators as msm_spectrum. */
msm_status msm_matrix_power(msm_ctx* ctx, const double* d_T, int64_t t_stride, int ld, const int32_t* d_n, int n_max,
                            int batch, int n_squarings, double* d_scratch, double* d_out);
msm_status msm_spectrum_powered(msm_ctx* ctx, const double* d_T, const double* d_T_power, int64_t t_stride, int ld,
                                const int32_t* d_n, int n_max, int batch, int p, int n_iter, int init, uint64_t seed,
                                int n_watch, void* d_workspace, double* d_ritz, double* d_pi, int64_t pi_stride,
                                double* d_change, int32_t* d_status, int n_its, const double* d_lags,
                                double* d_its_eig, double* d_its_ts, double freeze_tol, double* d_vecs, int n_vecs);

/* Reversible maximum-likelihood estimate: deeptime's MaximumLikelihoodMSM(reversible=True) as
 * called by _fit_msm_deeptime (S/markov_state_model/_msm_utils.py:210-262) and the lag selector
 * (S/markov_state_model/ck_its_selector.py:395-401), restated from the published fixed-point
 * iteration x_ij <- (c_ij + c_ji) / (c_i/x_i + c_j/x_j) on the row sums x_i, normalised every step,
 * until max_i |x_i - x_i'| / ((x_i + x_i')/2) <= maxerr (deeptime: 1e-8) or maxiter (1e6).
 * d_counts f64 [n, ld] must be a connected count matrix (e.g. ensure_connected_counts' result);
 * d_T f64 [n, ldt] row-stochastic with pi_i T_ij = pi_j T_ji, d_pi f64 [n] (may be NULL).
 * The convergence test polls the host (every 32, 64, ... 1024 iterations): the call synchronises the
 * stream and cannot be captured.  *h_iterations / *h_err (host, may be NULL) report what was run. */
msm_status msm_reversible_mle(msm_ctx* ctx, const double* d_counts, int n, int ld, double maxerr, int maxiter,
                              double* d_T, int ldt, double* d_pi, int* h_iterations, double* h_err);

/* The same estimate for `batch` matrices of RAW resampled counts in one launch, each with its own active set and its
 * own iteration count: what KineticImportanceScore._rebuild_msm (S/conformations/kinetic_importance.py:278-315) does
 * per bootstrap sample -- ensure_connected_counts (S/utils/msm_utils.py:129-167), then deeptime's
 * MaximumLikelihoodMSM(reversible=True), absent here (parity unpinned).  No host round trip; plain launch on the
 * context's stream, capturable once the scratch has been reserved by an eager call of the same shape.
 *   d_counts     int64 [batch, k, k], msm_combine_counts' output
 *   alpha        prior added to every cell of the active block (ensure_connected_counts: 1e-3), >= 0
 * Per matrix: the active set is {i : rowsum_i + colsum_i > 1e-12} in ascending order (n of them); the iteration of
 * msm_reversible_mle runs on C[active, active] + alpha from the row sums of C + C', normalised every step, and stops
 * at the FIRST iteration with max_i |x_i - x_i'| / ((x_i + x_i')/2) <= maxerr, or at maxiter (checked every
 * iteration, not in blocks as msm_reversible_mle does).
 *   d_T          f64, matrix b at d_T + b*t_stride with row stride ld >= k: the n x n estimate packed in the top-left
 *                corner, zeros in the rest of the k x k slot (the layout msm_spectrum takes with d_n = d_n_active)
 *   d_pi         f64 [batch, k]: the first n entries, 0 after them
 *   d_active     int32 [batch, k]: packed index -> state for the first n entries, -1 after them
 *   d_n_active   int32 [batch]
 *   d_iterations int32 [batch]
 *   d_err        f64 [batch]: the stopping measure of the last iteration
 * A matrix with an empty active set reports n = 0, 0 iterations, err = 0 and a zero slot.  A matrix that holds a
 * negative count, or whose iterate turns NaN, reports err = +inf (with a negative count: 0 iterations, zero slot and
 * zero pi); the other matrices of the batch are unaffected.
 * One workgroup of 1024 threads per matrix; all sums run in an order fixed by the matrix alone, so a matrix has the
 * same bits in any batch.  k <= msm_reversible_mle_batched_lds_max_n() keeps the symmetrised block in LDS; above,
 * it is streamed from slab b of the context scratch (msm_reversible_mle_batched_scratch_bytes tells the caller how
 * much a batch takes, so that it can split one).  k <= 2048 (MSM_ERR_UNSUPPORTED above). */
int msm_reversible_mle_batched_lds_max_n(void);
size_t msm_reversible_mle_batched_scratch_bytes(int k, int batch);
msm_status msm_reversible_mle_batched(msm_ctx* ctx, const int64_t* d_counts, int k, int batch, double alpha,
                                      double maxerr, int maxiter, double* d_T, int64_t t_stride, int ld, double* d_pi,
                                      int32_t* d_active, int32_t* d_n_active, int32_t* d_iterations, double* d_err);

/* Kinetic importance scores of a batch: KIS(i) = pi_i * sum_{m=1..k_slow} phi_m(i)^2 over the slow left eigenvectors
 * (KineticImportanceScore.compute, S/conformations/kinetic_importance.py:76-80), scattered back to the full state
 * space.
 *   d_vecs     f64 [batch, n_vecs, k]: msm_spectrum's d_vecs (row 0 the stationary vector), n_vecs >= k_slow + 1
 *   d_pi       f64 [batch, k], d_active int32 [batch, k], d_n_active int32 [batch]: packed as
 *              msm_reversible_mle_batched writes them
 *   d_scores   f64 [batch, k] OVERWRITTEN: scores[active[a]] = pi[a] * sum_m vecs[m][a]^2, 0 at inactive states
 *   d_info     int32 [batch] OVERWRITTEN: 0; 1 when n_active <= k_slow (all scores 0); 2 when a needed vector row
 *              holds NaN (a complex pair; the scores of such entries stay 0) */
msm_status msm_kis_scores(msm_ctx* ctx, const double* d_vecs, int n_vecs, int k, int batch, const double* d_pi,
                          const int32_t* d_active, const int32_t* d_n_active, int k_slow, double* d_scores,
                          int32_t* d_info);

/* Posterior samples of a mode-1 estimate for the implied-timescale confidence intervals
 * (ITSMixin._its_compute_for_single_lag, S/markov_state_model/_its.py:272-357, which asks
 * deeptime's BayesianMSM for n_samples matrices; that sampler's stream is not reproducible, so
 * this draws from the closed-form posterior of the estimator msm_transition_matrix implements):
 * row i of every sample ~ Dirichlet(C[active[i], active[:]] + alpha), rows independent.
 * d_counts / d_active / d_n_active as for msm_transition_matrix mode 1.  Sample s (numbered
 * first_sample + s) is written packed (n_active x n_active, row stride ld) at d_T + s*t_stride:
 * the layout msm_spectrum's batch takes.  Variates are Philox4x32-10 keyed by `seed` with counter
 * (column, row, sample number, attempt): a cell does not depend on the batch it is drawn in. */
msm_status msm_sample_transition_matrices(msm_ctx* ctx, const void* d_counts, int counts_are_f64, int k,
                                          const int32_t* d_active, const int32_t* d_n_active, double alpha,
                                          uint64_t seed, int first_sample, int n_samples, double* d_T,
                                          int64_t t_stride, int ld);

/* Posterior samples of the REVERSIBLE estimate for the same confidence intervals: the law of deeptime's
 * BayesianMSM(lagtime, n_samples) with its default reversible=True, which ITSMixin._its_compute_for_single_lag
 * fits (S/markov_state_model/_its.py:289-312) and _summarize_its_stats (:543-668) summarises.  deeptime is absent
 * (parity unpinned); the law is the published one, Trendelkamp-Schroer, Wu, Paul and Noe, J. Chem. Phys. 143,
 * 174101 (2015): symmetric X >= 0 with T_ij = x_ij / x_i, pi_i = x_i / sum x and
 *   p(X | C) ~ prod_i x_ii^(C_ii - 1) prod_{i<j} x_ij^(C_ij + C_ji - 1) prod_i x_i^(-c_i),   c_i = sum_j C_ij;
 * cells with C_ij + C_ji == 0 are exactly 0 in every sample.  One independent Gibbs / Metropolis chain per sample
 * (csrc/revposterior.hip describes the updates, the scan and the 1e-280 floor), started from X0 = diag(pi0) T0
 * and run for n_sweeps sweeps.
 * d_counts f64 [n, ld]: non-negative counts with the caller's prior already added (e.g. ensure_connected_counts'
 * result); d_T0 f64 [n, ld] and d_pi0 f64 [n]: the reversible maximum-likelihood estimate of the same counts
 * (msm_reversible_mle).  Sample s (numbered first_sample + s) is written at d_T + s*t_stride with row stride ldt,
 * the layout msm_spectrum's batch takes, and satisfies pi_i T_ij = pi_j T_ji with its own pi, written to
 * d_pi f64 [n_samples, n] (may be NULL).  Variates are Philox4x32-10 keyed by `seed` with counter (cell, sample
 * number, sweep, attempt): a sample does not depend on the batch it is drawn in.  Plain launches on the context's
 * stream, capturable.  n * 8 bytes must fit the 96 KB LDS table (MSM_ERR_UNSUPPORTED above);
 * n_samples <= 65535 per call. */
msm_status msm_sample_reversible_transition_matrices(msm_ctx* ctx, const double* d_counts, int n, int ld,
                                                     const double* d_T0, const double* d_pi0, uint64_t seed,
                                                     int first_sample, int n_samples, int n_sweeps, double* d_T,
                                                     int64_t t_stride, int ldt, double* d_pi);

/* The regularised active-set counts of ensure_connected_counts (S/utils/msm_utils.py:129-167) from the outputs of
 * msm_transition_matrix mode 1: d_out f64 [n_active, n_active] contiguous,
 * d_out[a, b] = counts[active[a], active[b]] + alpha.  Feeds msm_reversible_mle and the sampler above. */
msm_status msm_active_counts(msm_ctx* ctx, const void* d_counts, int counts_are_f64, int k, const int32_t* d_active,
                             const int32_t* d_n_active, double alpha, double* d_out);

/* One Philox4x32-10 block (known-answer test of the generator): d_out uint32 [4]. */
msm_status msm_philox4x32(msm_ctx* ctx, uint64_t key, const uint32_t counter[4], uint32_t* d_out);

/* ---- Chapman-Kolmogorov test ---------------------------------------------
 * msm_gemm_f64: C (m x n) = A (m x k) . B (k x n), row-major fp64 on the matrix cores; every
 * output element is the ascending-k FMA chain from +0 (bit-reproducible).  C must not alias
 * A or B.  Building block of the matrix powers below.
 *
 * msm_ck_test replaces the numerics of ck_error / _multinomial_rms_se / decide_ck
 * (S/validation/ck_rule.py:36-63, 71-117) and of _ck_on_trajs (S/markov_state_model/
 * ck_runner.py:155-176): for every factor f = h_factors[i]
 *   d_mse[i]   = mean((T1^f - Tk[i])^2)                         (RMS error = sqrt of it)
 *   d_noise[i] = sqrt(mean_i(sum_j p_ij (1 - p_ij) / N_i / n)),  p = Tk[i], N = row counts of
 *                the lag-f*tau count matrix (N_i <= 0 or non-finite -> 1); skipped when
 *                d_rowcounts / d_noise are NULL
 * d_T1 f64 [n, ld1]; d_Tk f64 [n_factors][tk_stride] with row stride ldk; d_rowcounts f64
 * [n_factors][rc_stride].  T1^f is formed by f-1 right-multiplications with T1. */
msm_status msm_gemm_f64(msm_ctx* ctx, int m, int n, int k, const double* d_A, int64_t lda,
                        const double* d_B, int64_t ldb, double* d_C, int64_t ldc);
msm_status msm_ck_test(msm_ctx* ctx, const double* d_T1, int64_t ld1, const double* d_Tk,
                       int64_t tk_stride, int64_t ldk, int n, const int32_t* h_factors, int n_factors,
                       const double* d_rowcounts, int64_t rc_stride, double* d_mse, double* d_noise);

/* d_out f64 [3] = { sum |P - Q|, sum |Q|, sum (P - Q)^2 } over the n x m entries (fixed order).
 * The relative L1 error of the lag selector's CK test is out[0] / out[1]
 * (_compute_ck_error, S/markov_state_model/ck_its_selector.py:211-226). */
msm_status msm_diff_norms(msm_ctx* ctx, const double* d_P, int64_t ldp, const double* d_Q, int64_t ldq, int n, int m,
                          double* d_out);

/* Exact order statistics: h_out[q] = the h_ranks[q]-th smallest (0-based) of the n strided samples, by radix
 * selection on the order-preserving integer image of the doubles (six 12-bit histogram passes per rank; no
 * sort).  Feeds the quantile rules of the free-energy grids (mquantiles / iqr in generate_2d_fes,
 * S/markov_state_model/free_energy.py:494-590) and medians.  NaN samples of either sign sort last, as in np.sort (a
 * rank among them returns a NaN); -0.0 sorts before +0.0.  Polls the host
 * between passes: synchronises the stream, cannot be captured. */
msm_status msm_order_statistics(msm_ctx* ctx, const double* d_x, int64_t stride, int64_t n, const int64_t* h_ranks,
                                int n_ranks, double* h_out);

/* ---- free-energy surfaces (S/analysis/fes.py) -----------------------------
 * msm_weighted_stats: d_out6 = {sum w, sum w^2, weighted mean, weighted variance (around that
 *   mean, / sum w), min, max} of the strided coordinate x[i * stride]; d_w NULL = unit weights
 *   (np.average twice, _compute_bandwidth :142-173; data range of np.histogram2d).
 * msm_hist2d: np.histogram2d(x, y, bins=[nx, ny], weights=w) on the given edges (:241-249):
 *   bin = searchsorted(edges, v, 'right') - 1, last edge inclusive, values outside or NaN
 *   dropped.  d_hist f64 [nx, ny].  Weighted sums run in 2^e fixed point (e from n * w_absmax,
 *   w_absmax >= max |w|): independent of scheduling, exact to 2^-e per frame.
 * msm_smooth_sparse_bins: bins < min_count are raised to max(mean of the 8 neighbours with
 *   replicated edges, min_count) when that mean is > 0 (:270-292); d_out != d_hist;
 *   *d_n_smoothed = number of changed bins.  msm_scale_to_total rescales to a given sum
 *   (the reference restores the raw total only when something was smoothed, :254-258).
 * msm_fes_finalize: F = -kT ln(h / sum h) - min (:570-599).  *d_status: 0 ok, bit 0 non-finite
 *   entry, bit 1 total <= 0, bit 2 entry <= 0 (the reference raises for each).
 * msm_kde2d: density[i][j] = 1/(2 pi bw_x bw_y) sum_k w_k w_scale exp(-((xc_i - x_k)/bw_x)^2/2)
 *   exp(-((yc_j - y_k)/bw_y)^2/2) on the matrix cores (:176-238); d_w NULL = all weights
 *   w_scale.  periodic bit 0 / bit 1: the x / y difference is wrapped to [-pi, pi) first (wrapped
 *   Gaussian on the torus: periodic_kde_2d, S/markov_state_model/free_energy.py:321-360). */
msm_status msm_weighted_stats(msm_ctx* ctx, const double* d_x, int64_t stride, int64_t n,
                              const double* d_w, double* d_out6);
msm_status msm_hist2d(msm_ctx* ctx, const double* d_x, int64_t sx, const double* d_y, int64_t sy,
                      int64_t n, const double* d_w, double w_absmax, const double* d_xedges, int nx,
                      const double* d_yedges, int ny, double* d_hist);
msm_status msm_smooth_sparse_bins(msm_ctx* ctx, const double* d_hist, int nx, int ny,
                                  double min_count, double* d_out, int32_t* d_n_smoothed);
msm_status msm_scale_to_total(msm_ctx* ctx, double* d_v, int n, double total);
msm_status msm_fes_finalize(msm_ctx* ctx, const double* d_hist, int n_cells, double kT,
                            double* d_F, int32_t* d_status);
msm_status msm_kde2d(msm_ctx* ctx, const double* d_x, int64_t sx, const double* d_y, int64_t sy,
                     int64_t n, const double* d_w, double w_scale, const double* d_xcenters, int nx,
                     const double* d_ycenters, int ny, double bw_x, double bw_y, int periodic, double* d_density);

/* d_out[t] = np.clip(x[t], lo, hi) (mode 1) or ((x[t] - lo) % (hi - lo)) + lo with numpy's remainder (mode 2):
 * the sample preparation of generate_2d_fes (S/markov_state_model/free_energy.py:494-556). */
msm_status msm_clip_or_wrap(msm_ctx* ctx, const double* d_x, int64_t stride, int64_t n, double lo, double hi, int mode,
                            double* d_out);

/* d_out[t] = d_table[d_idx[t]], 0 for an index outside [0, m): the frame weights pi[state] of the MSM-reweighted
 * free-energy surface (FESCalculator.calculate_fes, S/markov_state_model/free_energy.py:1011). */
msm_status msm_gather_f64(msm_ctx* ctx, const double* d_table, int m, const int32_t* d_idx, int64_t n, double* d_out);

/* ---- dense solves on T: committors, reactive flux, lumping, MFPT ---------------------------
 * msm_solve_f64: A X = B by Gaussian elimination with partial pivoting (first maximal pivot),
 *   one workgroup; d_A [n, lda] is overwritten by the factors, d_B [n, ldb] by X.
 *   *d_info = 0, or j + 1 when column j has no non-zero pivot (singular).
 * msm_reactive_flux replaces the numerics TPTMixin gets from deeptime (S/markov_state_model/
 *   _tpt.py:39-160, 255-347): d_role[i] = 0 intermediate, 1 source A, 2 sink B;
 *   q+ : (T - I) q = 0 on intermediates, q = 0 on A, 1 on B;   q- : the same for the time-reversed
 *   chain pi_j T_ji / pi_i with 1 on A, 0 on B;   gross f_ij = pi_i q-_i T_ij q+_j (i != j);
 *   net = max(0, f_ij - f_ji);   d_totals = {F = sum_{i in A, j not in A} f_ij, Z = sum_i pi_i q-_i,
 *   rate F / Z, mfpt Z / F}.  d_info int32 [2] (forward, backward solve).  d_gross / d_net /
 *   d_totals may be NULL together (committors only).
 * msm_lump_macro: lump_micro_to_macro_T + compute_macro_populations (S/markov_state_model/
 *   _msm_utils.py:103-135): F_AB = sum_{i in A, j in B} pi_i T_ij, T_macro = F / rowsum (zero rows
 *   stay zero), pi_macro[A] = sum_{i in A} pi_i renormalised.
 * msm_macro_mfpt: compute_macro_mfpt (:138-160): for every target j solve (I - Q_j) t = 1 with
 *   row / column j removed; d_mfpt f64 [n, n] (column j = times into j, diagonal 0); d_info [n]. */
msm_status msm_solve_f64(msm_ctx* ctx, int n, int nrhs, double* d_A, int64_t lda, double* d_B,
                         int64_t ldb, int32_t* d_info);
msm_status msm_reactive_flux(msm_ctx* ctx, const double* d_T, int64_t ldt, const double* d_pi,
                             const int32_t* d_role, int n, double* d_qplus, double* d_qminus,
                             double* d_gross, double* d_net, double* d_totals, int32_t* d_info);
msm_status msm_lump_macro(msm_ctx* ctx, const double* d_T, int64_t ldt, const double* d_pi,
                          const int32_t* d_macro, int n, int n_macro, double* d_T_macro,
                          double* d_pi_macro);
msm_status msm_macro_mfpt(msm_ctx* ctx, const double* d_T, int64_t ldt, int n, double* d_mfpt,
                          int32_t* d_info);

/* ---- dominant reactive pathways through the net flux (csrc/pathways.hip) ----------------------------
 * Replaces the host walk behind flux.pathways(fraction, maxiter) in TPTAnalysis.analyze
 * (S/conformations/tpt_analysis.py:122-135) and TPTMixin.pathway_decomposition (S/markov_state_model/
 * _tpt.py:162-211); the rule is that of pmarlo_amd/markov_state_model/tpt.py::pathway_decomposition / _widest_path.
 *
 * Work matrix G of order N = n + 2: G[:n, :n] = d_net (f64 [n, ldn], finite and >= 0); the virtual source n has
 * G[n][a] = sum_j net[a][j] for every source a (d_role[a] == 1), the virtual sink n + 1 has G[b][n+1] =
 * sum_i net[i][b] for every sink b (d_role[b] == 2); total = sum_a G[n][a].  Each of the three sums is ONE
 * sequential fp64 chain in ascending index.
 * One path is a max-min Dijkstra from n to n + 1: width[n] = +inf, every other width 0; pop the not-done node i of
 * largest width, the lowest index on equal widths; no path when that width is 0; stop when n + 1 is popped;
 * otherwise, for every not-done j with min(width[i], G[i][j]) > width[j] (strictly), set width[j] to it and
 * prev[j] = i.  cap = width[n+1].  The decomposition ends with status NO_PATH when there is no path or
 * cap <= 1e-14 * total.  Otherwise G[a][b] = max(0.0, G[a][b] - cap) along the path, the path without its virtual
 * ends is appended, got += cap, and the loop continues while
 *     n_paths < maxiter  &&  total > 0  &&  got < fraction * total * (1.0 - 1e-14)      (products left to right);
 * when it does not, the status is NO_PATH for total <= 0, else FRACTION for the collected share, else MAXITER.
 * Only min, max, compares, one subtraction and one addition touch the data: results are fixed bit for bit.
 *
 * The entry is resumable, so that no launch runs long: the state (G, got, total, path count, status) lives in
 * d_work (msm_reactive_pathways_work_bytes(n) bytes, 64-byte header + G).
 *   msm_reactive_pathways_begin builds G and the header and clears the outputs; header.bad != 0 afterwards
 *     means d_net holds a negative, infinite or NaN entry (the caller must not run then).
 *   msm_reactive_pathways_run is ONE launch of ONE workgroup that takes at most launch_paths paths (0: the default
 *     msm_reactive_pathways_launch_paths(n) = MSM_PATHWAYS_LAUNCH_POPS / (n + 2), at least 1: a search pops at
 *     most n + 2 nodes) and returns; the caller reads the first 32 bytes of d_work, {f64 got, f64 total,
 *     i32 n_paths, i32 status, i32 bad, i32 pad}, and calls again while status == MSM_PATHWAYS_RUNNING, with the
 *     same fraction / maxiter / keep and outputs.
 * Outputs: d_caps f64 [maxiter], entry p the capacity of path p, for all paths found; d_paths int32 [keep, n] and
 * d_len int32 [keep]: the nodes of the first `keep` paths, padded with -1 (a path visits a node at most once).
 * n <= MSM_PATHWAYS_MAX_N, above: MSM_ERR_UNSUPPORTED naming both numbers. */
#define MSM_PATHWAYS_MAX_N 2048
#define MSM_PATHWAYS_LAUNCH_POPS 131072   /* node pops a launch may take at most */
#define MSM_PATHWAYS_RUNNING 0
#define MSM_PATHWAYS_FRACTION 1           /* the requested share of the total flux is collected */
#define MSM_PATHWAYS_NO_PATH 2            /* no path left, or its capacity is under the floor */
#define MSM_PATHWAYS_MAXITER 3            /* maxiter paths were taken */
size_t msm_reactive_pathways_work_bytes(int n);
int msm_reactive_pathways_launch_paths(int n);
msm_status msm_reactive_pathways_begin(msm_ctx* ctx, const double* d_net, int64_t ldn, const int32_t* d_role, int n,
                                       int maxiter, int keep, void* d_work, double* d_caps, int32_t* d_paths,
                                       int32_t* d_len);
msm_status msm_reactive_pathways_run(msm_ctx* ctx, void* d_work, int n, double fraction, int maxiter, int keep,
                                     int launch_paths, double* d_caps, int32_t* d_paths, int32_t* d_len);

/* ---- effective count matrix (csrc/effective.hip) ---------------------------------------------------
 * count_mode = "effective" of the reference's counting backend (deeptime 0.4.5 TransitionCountEstimator;
 * deeptime.markov.tools.estimation.effective_count_matrix / statistical_inefficiencies, after Noe 2015), written
 * from the documented algorithm.  Parity with deeptime's own output is NOT pinned; the tests hold the kernels to a
 * numpy / Python restatement of the rule below (tests/_effective_ref.py).
 *
 * d_labels int32 [n], n < 2^31.  Segments [start, stop) on the host: ascending, disjoint, inside [0, n], else
 * MSM_ERR_INVALID (n_seg = 0: one segment [0, n)); every segment is one trajectory.  A start frame is a frame t of
 * a segment with t + lag < stop and labels[t], labels[t + lag] in [0, k).  C (d_counts, int64 [k, k]) is
 * msm_count_transitions over the same segments with stride 1.
 * Row i: per segment the time-ordered targets labels[t + lag] of its start frames with labels[t] == i, one
 * sub-sequence each (a segment without such a frame gives none).  N_i = sum of their lengths (the row sum of C),
 * M_i = the longest.  For a cell c = C_ij > 0, x = (target == j) along row i, and for l = 0 .. M_i - 1, summed
 * over the sub-sequences of length Nx:
 *     n_l = sum max(Nx - l, 0),  S_l = sum_p x_p x_(p+l),  A_l = sum_(p < Nx - l) x_p,  B_l = sum_(p >= l) x_p,
 *     Q_l = S_l N_i^2 - c N_i (A_l + B_l) + c^2 n_l          (exact, 128-bit integers)
 * The truncation lag l* is the first l with Q_l <= 0, decided on the integer (deeptime compares a float), M_i
 * when there is none.  corrsum = sum_(l = 1 .. l* - 1) Q_l (M_i - l) / (N_i^2 n_l M_i), in fp64 in ascending l;
 * si_ij = 1 / (1 + 2 mact corrsum N_i / c).  A row with a single target has Q_0 = 0: l* = 0 and si = 1.
 * average: ROW  Ceff_ij = w_i C_ij with w_i = sum_j C_ij si_ij / N_i (deeptime's estimator, mact = 1);
 *          ALL  one weight sum C si / sum C;   NONE  Ceff = C o si.
 * Outputs, all OVERWRITTEN: d_ceff f64 [k, k], d_si f64 [k, k] (0 where C = 0), d_counts int64 [k, k], d_trunc
 * int32 [k, k] = l* (0 where C = 0).
 *
 * One workgroup per cell walks the lags in blocks of MSM_EFF_LAG_BLOCK with integer LDS histograms; a launch
 * advances every unfinished cell by at most blocks_per_launch blocks (0: MSM_EFF_BLOCKS_PER_LAUNCH), writes the
 * cell's state {corrsum, next lag, done} back to d_work and counts the cells it left unfinished; the host reads
 * that count and launches again until it is zero (not capturable).  An autocorrelation that never decays costs
 * O(c^2) pair visits by definition: they arrive as many bounded launches.  The cut between launches changes no
 * operation: the same bytes for every blocks_per_launch and on every run.  *h_launches (may be NULL): how many
 * such launches ran.  d_work: msm_effective_counts_work_bytes(n, k, n_seg) bytes; the grouping also uses the
 * context scratch (msm_group_by_label). */
#define MSM_EFF_LAG_BLOCK 256
#define MSM_EFF_BLOCKS_PER_LAUNCH 8
#define MSM_EFF_AVERAGE_ROW 0
#define MSM_EFF_AVERAGE_ALL 1
#define MSM_EFF_AVERAGE_NONE 2
size_t msm_effective_counts_work_bytes(int64_t n, int k, int n_seg);
msm_status msm_effective_counts(msm_ctx* ctx, const int32_t* d_labels, int64_t n, const int64_t* h_seg_start,
                                const int64_t* h_seg_stop, int n_seg, int lag, int k, int average, double mact,
                                int blocks_per_launch, void* d_work, size_t work_bytes, double* d_ceff, double* d_si,
                                int64_t* d_counts, int32_t* d_trunc, int64_t* h_launches);

/* ---- trajectory bootstrap in batch (csrc/bootstrap.hip) ----------------------------------------
 * The device side of UncertaintyQuantifier (S/conformations/uncertainty.py:31-261): every bootstrap sample
 * resamples whole trajectories with replacement and rebuilds the MSM (_rebuild_msm, :506-530).  Counts are
 * additive over trajectories, so trajectory s is counted once (msm_count_transitions into slice s of an int64
 * [n_seg, k*k] buffer) and sample b is the integer combination below; the committor systems of all samples are
 * then solved by one launch.
 * msm_combine_counts: d_seg_counts int64 [n_seg, cells]; d_mult int32 [n_boot, ld_mult], column s = how often
 *   trajectory s occurs in sample b (ld_mult >= n_seg lets a chunk of trajectories point into a wider table);
 *   d_counts int64 [n_boot, cells] OVERWRITTEN with C_b = sum_s mult[b, s] * C_s, or ADDED TO when accumulate != 0
 *   (further chunks of trajectories).  Integer arithmetic: exact, no atomics.  1 <= n_seg <= MSM_COMBINE_MAX_SEG
 *   per call (the values of a cell stay in registers while the samples stream past).
 * msm_row_normalise_batched: d_counts int64 [batch, k, k] -> d_T f64 [batch, k, k] OVERWRITTEN, T = C / rowsum as
 *   the IEEE double quotient of the two integers, all-zero rows stay zero (msm_transition_matrix mode 0;
 *   uncertainty.py:519-522); d_rowsum int64 [batch, k] OVERWRITTEN.
 * msm_reactive_flux_batched: msm_reactive_flux for `batch` matrices (sample b at d_T + b*t_stride, row stride ldt),
 *   d_pi f64 [batch, n], ONE d_role int32 [n] for all; d_qplus / d_qminus f64 [batch, n] OVERWRITTEN (may be NULL
 *   together), d_totals f64 [batch, 4] = {F, Z, rate, mfpt} OVERWRITTEN (may be NULL when the committors are asked
 *   for), d_info int32 [batch, 2] (forward, backward solve) OVERWRITTEN.  Gross and net flux are not written.
 *   One workgroup per sample.  n <= MSM_FLUX_LDS_MAX_N: the system matrix and its right-hand side stay in LDS,
 *   (n*n + n) * 8 bytes <= 128 KiB of the 160 KiB a gfx950 workgroup can have; above, in slab b of the context
 *   scratch (msm_reactive_flux_batched_scratch_bytes tells the caller how much a batch takes, so that it can
 *   split one).  Same pivot rule and per-element fma recurrences as msm_solve_f64 on both paths: the committors
 *   of sample b have the bits msm_reactive_flux returns for that matrix alone; the totals are summed in a fixed
 *   order of their own.  A singular system sets d_info of its sample only (committors and totals of that sample
 *   NaN); the other samples are unaffected. */
#define MSM_COMBINE_MAX_SEG 32      /* trajectories per msm_combine_counts call */
#define MSM_FLUX_LDS_MAX_N 127      /* largest n of the LDS-resident committor solve */
msm_status msm_combine_counts(msm_ctx* ctx, const int64_t* d_seg_counts, const int32_t* d_mult, int64_t ld_mult,
                              int n_seg, int n_boot, int64_t cells, int64_t* d_counts, int accumulate);
msm_status msm_row_normalise_batched(msm_ctx* ctx, const int64_t* d_counts, int k, int batch, double* d_T,
                                     int64_t* d_rowsum);
size_t msm_reactive_flux_batched_scratch_bytes(int n, int batch, int want_committors);
msm_status msm_reactive_flux_batched(msm_ctx* ctx, const double* d_T, int64_t t_stride, int64_t ldt,
                                     const double* d_pi, const int32_t* d_role, int n, int batch, double* d_qplus,
                                     double* d_qminus, double* d_totals, int32_t* d_info);

/* ---- silhouette score (n_states = "auto") ---------------------------------------------------
 * Replaces sklearn.metrics.silhouette_score in _auto_select_n_states (S/markov_state_model/
 * clustering.py:156-233).  d_x f64 [n, ld]: the points SORTED BY CLUSTER, cluster c = rows
 * [h_offsets[c], h_offsets[c+1]); 2 <= k <= 32.  d_samples f64 [n]: s_i = (b_i - a_i) / max(a_i,
 * b_i) (0 for singleton clusters); *d_score = mean s_i.
 * NaN rule, the one of msm_silhouette_samples below: non-finite coordinates are not dropped, the
 * minimum in b_i and the maximum in the denominator keep NaN, and the score is then NaN. */
msm_status msm_silhouette(msm_ctx* ctx, const double* d_x, int64_t n, int d, int64_t ld,
                          const int64_t* h_offsets, int k, double* d_samples, double* d_score);

/* ---- silhouette samples: any cluster count, any n < 2^31 --------------------------------------
 * sklearn.metrics.silhouette_samples / silhouette_score (Euclidean).  d_x f64 [n, ld] in frame
 * order, 1 <= d <= MSM_REP_MAX_D; d_labels int32 [n] on the device, dense ids 0 .. k-1 (an id
 * may be unused), 2 <= k <= n - 1; violations, a label outside [0, k) included, return
 * MSM_ERR_INVALID.  d_samples f64 [n] in frame order: s_i = (b_i - a_i) / max(a_i, b_i), 0 for
 * the member of a singleton cluster and where max(a_i, b_i) = 0; unused ids take no part in
 * b_i.  *d_score = mean s_i.
 * NaN rule: a_i and the cluster means are ordinary IEEE sums; b_i is a minimum over the other
 * clusters that have a member (decided by the counts) and max(a_i, b_i) a maximum, both of which
 * keep a NaN operand; s_i = 0 only for a singleton, where no other cluster has a member and where
 * max(a_i, b_i) = 0, otherwise (b_i - a_i) / max(a_i, b_i) as IEEE gives it.  One frame with a
 * NaN coordinate so makes s_i NaN for itself, its cluster and every frame whose b_i would have
 * to look at that cluster, and the score NaN: sklearn refuses such input, this says so in the
 * result.  Finite input is untouched by the rule.
 * The frames are grouped on the device (msm_group_by_label), every cluster is cut into segments
 * of MSM_SIL_SEG_LEN members, workgroups of MSM_SIL_TILE_I query frames x a group of segments
 * write one partial distance sum per (query, segment), and a fold adds a cluster's pieces in
 * segment order.  Distances are direct differences under the root.  No launch holds more than
 * max_products (i, j, feature) products (0: 2^36) unless one workgroup alone does; the cut
 * moves work between launches and changes no sum, and there are no atomics: the same bytes for
 * every cut and on every run.  d_work: msm_silhouette_workspace_bytes(n, d, k) bytes, at most
 * 256 MiB of partial sums plus 8 (k + 1) + 4 n bytes of grouping, whatever n and k are.
 * Reads the cluster sizes on the host: not capturable. */
#define MSM_SIL_SEG_LEN 1024
#define MSM_SIL_TILE_I 128
size_t msm_silhouette_workspace_bytes(int64_t n, int d, int k);
msm_status msm_silhouette_samples(msm_ctx* ctx, const double* d_x, int64_t n, int d, int64_t ld,
                                  const int32_t* d_labels, int k, void* d_work, size_t work_bytes,
                                  int64_t max_products, double* d_samples, double* d_score);

/* ---- regular-grid microstates (cluster_mode = "grid") -----------------------------------------
 * Replaces _GridDiscretizer._compute_indices / transform (S/analysis/discretize.py:552-583).
 * msm_grid_cells: d_flat[t] = sum_f idx_f * bins^(F-1-f), idx_f = clip(np.digitize(x[t][f],
 *   edges_f) - 1, 0, bins - 1); d_edges f64 [F][bins + 1] increasing; NaN -> last bin (as numpy).
 * msm_first_occurrence: d_first[c] = smallest frame index t with d_flat[t] == c, or -1 (the
 *   reference numbers states by order of first appearance).
 * msm_relabel: d_labels[t] = d_map[d_flat[t]]. */
msm_status msm_grid_cells(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                          const double* d_edges, int bins, int32_t* d_flat);
msm_status msm_first_occurrence(msm_ctx* ctx, const int32_t* d_flat, int64_t n, int n_cells,
                                int64_t* d_first);
msm_status msm_relabel(msm_ctx* ctx, const int32_t* d_flat, int64_t n, const int32_t* d_map, int n_cells,
                       int32_t* d_labels);

/* ---- representative frames of a state ---------------------------------------------------------
 * Replaces the per-state host loops of RepresentativePicker (S/conformations/
 * representative_picker.py) and _find_representatives (S/markov_state_model/_states.py:131-157).
 * Features d_x f64 [n, ld] with d <= MSM_REP_MAX_D (MSM_ERR_UNSUPPORTED above), labels int32 [n],
 * optional weights f64 [n] (NULL: w = 1), n < 2^31.  Every output is the same bytes on every run.
 * msm_group_by_label: d_members int32 [n] holds, for s = 0 .. k-1 in turn, the frames with label s
 *   in ascending order (np.where(labels == s)); state s = d_members[d_offsets[s] : d_offsets[s+1]],
 *   d_offsets int64 [k + 1].  Labels outside [0, k) belong to no state; d_members past
 *   d_offsets[k] is not written.  Frames are ranked in chunks of MSM_REP_GROUP_CHUNK.
 * msm_state_centroids: d_wsum[s] = sum w, d_centroid f64 [k, d] = sum w x / sum w over the members in
 *   a fixed order (0 for an empty state), d_flags int32 [k] = MSM_REP_FLAG_* bits of the state's
 *   weights (0 for an empty state).
 * msm_state_scores: d_scores f64, laid out like d_members.  MSM_REP_SCORE_CENTROID: |x_i - c_s|_2 for
 *   every member of every state (needs d_labels, d_centroid; the state list is not read).
 *   MSM_REP_SCORE_MEDOID: sum_j w^_j |x_i - x_j|_2 over the members j of i's state, w^ = w / sum w or
 *   1 / n_s, for the states h_states[0 .. n_states) only (needs d_wsum); tasks of MSM_REP_TILE_I rows
 *   against tiles of MSM_REP_TILE_J rows are built from h_offsets (the host copy of d_offsets) and
 *   uploaded, so this mode is not capturable.  Both take direct differences under the root.
 * msm_state_select: d_picks int32 [n_states, n_reps], frame indices, -1 where a state has fewer than
 *   n_reps members; h_states distinct.  MSM_REP_SELECT_SMALLEST: the members with the smallest
 *   (score, frame), in that order.  MSM_REP_SELECT_DIVERSE: the member with the smallest score
 *   (lowest frame on ties), then repeatedly the member farthest from everything picked so far
 *   (max-min walk, lowest frame on ties); d_scores holds centroid distances, d_mind f64 is workspace
 *   laid out like d_scores.  A NaN never wins (np.argmin / np.argmax of the reference's host loop
 *   return the first NaN): SMALLEST never picks a NaN score and ends the row in -1; in DIVERSE a NaN
 *   score never wins the start (member 0 if all are NaN) and a NaN distance to a pick never wins a
 *   round, the row ending in -1 once nothing else is left.  Uploads the state list: not capturable. */
#define MSM_REP_MAX_D 256
#define MSM_REP_GROUP_CHUNK 1024
#define MSM_REP_TILE_I 128
#define MSM_REP_TILE_J 64
#define MSM_REP_FLAG_NONFINITE 1
#define MSM_REP_FLAG_NEGATIVE 2
#define MSM_REP_FLAG_NONPOSITIVE_SUM 4
#define MSM_REP_SCORE_CENTROID 0
#define MSM_REP_SCORE_MEDOID 1
#define MSM_REP_SELECT_SMALLEST 0
#define MSM_REP_SELECT_DIVERSE 1
msm_status msm_group_by_label(msm_ctx* ctx, const int32_t* d_labels, int64_t n, int k, int64_t* d_offsets,
                              int32_t* d_members);
msm_status msm_state_centroids(msm_ctx* ctx, const double* d_x, int64_t n, int d, int64_t ld, const double* d_w,
                               const int64_t* d_offsets, const int32_t* d_members, int k, double* d_centroid,
                               double* d_wsum, int32_t* d_flags);
msm_status msm_state_scores(msm_ctx* ctx, const double* d_x, int64_t n, int d, int64_t ld, const double* d_w,
                            const int32_t* d_labels, const int64_t* d_offsets, const int32_t* d_members, int k,
                            const double* d_centroid, const double* d_wsum, int mode, const int64_t* h_offsets,
                            const int32_t* h_states, int n_states, double* d_scores);
msm_status msm_state_select(msm_ctx* ctx, const double* d_x, int64_t n, int d, int64_t ld, const int64_t* d_offsets,
                            const int32_t* d_members, int k, const double* d_scores, double* d_mind, int mode,
                            const int32_t* h_states, int n_states, int n_reps, int32_t* d_picks);

/* ---- MBAR frame weights for multi-ensemble runs (csrc/mbar.hip) -------------------------------------
 * The multistate Bennett acceptance ratio estimator, written from Shirts & Chodera, J. Chem. Phys. 129, 124105
 * (2008); the reference snapshot holds no reweighter, so nothing is ported.  The tests hold the kernels to a numpy
 * restatement of the rule below (tests/_mbar_ref.py), run in 80-bit floats.
 *
 * d_u [K, ld] f32 / f64, state-major: u[k, n] is the reduced potential of frame n in sampled state k, ld >= N.
 * +inf is allowed (the frame is forbidden in that state); NaN and -inf are invalid.  d_f f64 [K] the current free
 * energies, d_lnN f64 [K] = ln N_k.  1 <= K <= MSM_MBAR_MAX_K (MSM_ERR_UNSUPPORTED above), 1 <= N.
 * msm_mbar_pass, per frame n, all in fp64:
 *     m_n = min_k u_kn                                   (the per-frame shift: a no-op on W, d_n shifts back)
 *     b_k = (f_k - (u_kn - m_n)) + lnN_k,   M = max_k b_k,   e_k = exp(b_k - M),   S = sum_k e_k  (ascending k)
 *     d_n = (M + log S) - m_n               = logsumexp_k (f_k + ln N_k - u_kn), the log mixture denominator
 *     W_kn = e_k * exp(-lnN_k) * (1 / S)    = exp(f_k - u_kn - d_n)
 *   and over the frames  s_k = sum_n W_kn,  G_ij = sum_n W_in W_jn,  obj = sum_n d_n.
 *   Outputs, all OVERWRITTEN: d_logden f64 [N] (may be NULL), d_s f64 [K], d_G f64 [K, K] (symmetric bit for bit;
 *   NULL when !want_gram), d_obj f64 [1].  d_status int32 [1] is OR-ed into (the caller clears it): bit
 *   MSM_MBAR_BAD_INPUT marks a NaN or -inf in u, bit MSM_MBAR_BAD_FRAME a frame whose d_n is not finite (forbidden in
 *   every state); such a frame adds nothing to s, G and obj, and the caller must not use the results.
 *   Launch shape: a workgroup of MSM_MBAR_THREADS lanes takes MSM_MBAR_THREADS frames per trip, one lane per frame,
 *   in a grid-stride loop; the rows of u are read coalesced.  The workgroup's W slab [K, trip] goes through LDS; lane
 *   k of every wave adds its wave's 64 columns of row k to s_k, and the upper 16 x 16 tiles of the Gram update (at most
 *   10 at K = 64) are spread over the four waves and formed by v_mfma_f64_16x16x4_f64 with the accumulators in
 *   registers.  want_gram = 0 skips the Gram work and returns the same d, s and obj bits.  No floating-point atomics:
 *   every workgroup writes its partial s, G, obj to the context scratch and a second launch adds them in ascending
 *   workgroup order, so the results are the same bits on every run.  max_workgroups caps the grid (0: as many as are
 *   resident at once, three per CU, fewer when the LDS slab leaves room for fewer; the same with and without G).
 * msm_mbar_plan: read-only; what msm_mbar_pass would launch for (K, N, dtype, max_workgroups) on this context:
 *   out[0] = frames per workgroup trip, out[1] = grid size, out[2] = LDS bytes, out[3] = Gram tiles.
 * msm_mbar_state_means: d_mean[k] = mean of u[k, n] over n in [h_offsets[k], h_offsets[k+1]), state k's own frames
 *   (frames are grouped by the state that drew them), one workgroup per state, fixed order: the solver's initial
 *   guess is f_k = mean_k - mean_0.  h_offsets int64 [K + 1] on the host, ascending, inside [0, N].
 * msm_mbar_newton_system: with N_k = d_Nk f64 [K], the reduced Newton system of the convex objective
 *   Phi(f) = obj - sum_k N_k f_k under the gauge f_0 = 0:  d_H f64 [K-1, K-1], H_ij = delta_ij N_i s_i -
 *   N_i N_j G_ij and d_g f64 [K-1], g_i = N_i (s_i - 1), i, j = 1 .. K-1.  msm_solve_f64 then solves H x = g in place.
 * msm_mbar_weights: unsampled target states, rows of d_ut [T, ld] f32 / f64, from the stored d_n:
 *   c_n = -u_tn - d_n,  f_t = -logsumexp_n c_n,  w_tn = exp(c_n - logsumexp_n c_n)  (sum_n w_tn = 1),
 *   ESS_t = 1 / sum_n w_tn^2 (Kish).  d_ft f64 [T], d_w f64 [T, N], d_ess f64 [T]; d_status as above
 *   (BAD_INPUT: NaN or -inf in u_t; BAD_FRAME: a target no frame reaches, f_t = +inf).  Fixed-order reductions.
 * msm_mbar_reduced_potentials: the replica-ladder case, d_u f64 [K, ld], u[k, n] = d_beta[k] * (d_energy[n] +
 *   d_bias[k, n]) (d_bias f64 [K, ldb], NULL: no bias). */
#define MSM_MBAR_MAX_K 64
#define MSM_MBAR_THREADS 256
#define MSM_MBAR_BAD_INPUT 1
#define MSM_MBAR_BAD_FRAME 2
msm_status msm_mbar_plan(msm_ctx* ctx, int K, int64_t N, msm_dtype dtype, int max_workgroups, int64_t out[4]);
msm_status msm_mbar_pass(msm_ctx* ctx, const void* d_u, msm_dtype dtype, int K, int64_t N, int64_t ld,
                         const double* d_f, const double* d_lnN, int want_gram, int max_workgroups, double* d_logden,
                         double* d_s, double* d_G, double* d_obj, int32_t* d_status);
msm_status msm_mbar_state_means(msm_ctx* ctx, const void* d_u, msm_dtype dtype, int K, int64_t N, int64_t ld,
                                const int64_t* h_offsets, double* d_mean);
msm_status msm_mbar_newton_system(msm_ctx* ctx, int K, const double* d_s, const double* d_G, const double* d_Nk,
                                  double* d_H, double* d_g);
msm_status msm_mbar_weights(msm_ctx* ctx, const void* d_ut, msm_dtype dtype, int T, int64_t N, int64_t ld,
                            const double* d_logden, double* d_ft, double* d_w, double* d_ess, int32_t* d_status);
msm_status msm_mbar_reduced_potentials(msm_ctx* ctx, const double* d_energy, const double* d_bias, int64_t ldb,
                                       const double* d_beta, int K, int64_t N, int64_t ld, double* d_u);

/* ---- TRAM: multi-ensemble Markov models and frame weights (csrc/tram.hip) ----------------------------
 * The transition-based reweighting analysis method, written from Wu, Paul, Wehmeyer, Noe, PNAS 113, E3221 (2016);
 * the reference snapshot holds no reweighter, so nothing is ported.  The tests hold the kernels to a numpy
 * restatement of the rule below (tests/_tram_ref.py), run in 80-bit floats.
 *
 * K thermodynamic states (1 <= K <= MSM_MBAR_MAX_K), m Markov states (1 <= m <= MSM_TRAM_MAX_STATES), N frames;
 * MSM_ERR_UNSUPPORTED above either limit.  d_u [K, ld] f32 / f64 as in MBAR (+inf allowed, NaN and -inf invalid),
 * with the frames GROUPED BY MARKOV STATE: state i owns the frames [offsets[i], offsets[i+1]), every state has one.
 * d_S f64 [K, m, m], S^k = C^k + C^k' of the lag-tau counts; d_N f64 [K, m], N_i^k = frames of state i drawn in
 * ensemble k; d_col f64 [K, m], col_i^k = sum_j C^k_ji.  The pair (k, i) is active iff N_i^k > 0; S is zero in the
 * rows and columns of inactive pairs.  The unknowns: d_f f64 [K, m], the local free energies, and d_v f64 [K, m],
 * the Lagrange multipliers; g_i^k = ln v_i^k + f_i^k (-inf where v = 0).  One iteration:
 *   1. v_i^k   = sum_j S_ij / (1 + exp(g_j - g_i))                      (old f, old v)
 *   2. R_i^k   = sum_j S_ij / (1 + exp(g_i - g_j)) + (N_i^k - col_i^k)  (old f, new v),   tab_i^k = ln R_i^k + f_i^k
 *   3. per frame n of state i:  m_n = min_l u_ln,  a_l = tab_i^l - (u_ln - m_n),  M = max_l a_l,
 *      e_l = exp(a_l - M),  S = sum_l e_l (ascending l),  d_n = (M + log S) - m_n,  r_l = e_l * (1 / S);
 *      s_i^k = sum of r_k over the frames of state i
 *   4. f_i^k   = tab_i^k - ln s_i^k  on the active pairs
 *   5. f      -= its minimum over the active pairs;  err = max |f_new - f_old| over them;  g = ln v + f_new.
 *   Inactive pairs: v = R = 0, tab = g = -inf, f untouched; they add nothing to a frame's sum.
 * msm_tram_rows: steps 1 and 2 are one kernel.  mode MSM_TRAM_ROWS_MULTIPLIERS: d_out = v, d_lnout = ln v + f;
 *   mode MSM_TRAM_ROWS_COUNTS: d_out = R, d_lnout = tab.  d_g f64 [K, m] is read (never an output of the same call).
 *   One wave per row (k, i): lane l adds the columns l, l + 64, .. in ascending order, then a fixed shuffle tree;
 *   the S row is read coalesced; where S_ij = 0 there is no exp and no division.
 * msm_tram_pass: step 3.  The work unit is (state, segment of MSM_TRAM_SEGMENT frames of its range), one lane per
 *   frame, fp64 throughout; the tables that name the units are on the device and built once per problem:
 *   d_offsets int64 [m + 1]; d_unit_ptr int64 [m + 1], state i owns the units [unit_ptr[i], unit_ptr[i+1]), one per
 *   started segment; d_unit_state int32 [units].  A unit's K sums go to the context scratch, a second launch adds a
 *   state's units in ascending order into d_s f64 [K, m]: no floating-point atomics, and the same bits on every run
 *   and for every max_workgroups (0: as many workgroups as are resident at once).  d_logden f64 [N] (may be NULL)
 *   receives d_n.  d_status int32 [1] is OR-ed into as in MBAR: MSM_MBAR_BAD_INPUT for a NaN or -inf in u,
 *   MSM_MBAR_BAD_FRAME for a frame without a finite a_l (it adds nothing to s).  A unit whose table entries do not
 *   describe frames of [0, N) is empty.
 * msm_tram_update: steps 4 and 5 by one workgroup; d_f is updated in place, d_g and d_err f64 [1] are written.
 * msm_tram_iterations: n_iterations iterations enqueued back to back, nothing read back in between; every launch is
 *   bounded.  d_work f64 [5 K m] holds g, the g of step 2, R, tab and s (in that order) and is scratch otherwise;
 *   g is rebuilt from (f, v) at the start, with the bits step 5 leaves.  d_logden (may be NULL) receives the d_n of
 *   the last iteration's pass, d_err the err of the last iteration.
 * msm_tram_transition_matrices: for ensemble k (k = -1: all K, d_P f64 [K, m, m]; else d_P f64 [m, m]):
 *   p_ij = S_ij / (v_i + v_j exp(f_j - f_i)) for i != j among the active states; when the largest off-diagonal row
 *   sum exceeds 1 (short of convergence only) every off-diagonal entry is divided by it, which keeps detailed
 *   balance; p_ii = 1 - sum_{j != i} p_ij.  Rows and columns of inactive states are zero.  d_rowsum f64 [K, m] is
 *   scratch.  One workgroup per ensemble, one wave per row, sums in a fixed order.
 * msm_tram_plan: read-only; what msm_tram_pass would launch for state ranges h_offsets int64 [m + 1] (host):
 *   out[0] = segment length, out[1] = units, out[2] = grid size, out[3] = LDS bytes, out[4] = workgroups of a
 *   msm_tram_rows launch. */
#define MSM_TRAM_MAX_STATES 2048
#define MSM_TRAM_SEGMENT 256
#define MSM_TRAM_ROWS_MULTIPLIERS 0
#define MSM_TRAM_ROWS_COUNTS 1
msm_status msm_tram_plan(msm_ctx* ctx, int K, int m, const int64_t* h_offsets, int max_workgroups, int64_t out[5]);
msm_status msm_tram_rows(msm_ctx* ctx, int K, int m, const double* d_S, const double* d_g, const double* d_f,
                         const double* d_N, const double* d_col, int mode, double* d_out, double* d_lnout);
msm_status msm_tram_pass(msm_ctx* ctx, const void* d_u, msm_dtype dtype, int K, int m, int64_t N, int64_t ld,
                         const int64_t* d_offsets, const int64_t* d_unit_ptr, const int32_t* d_unit_state,
                         int64_t units, const double* d_tab, int max_workgroups, double* d_logden, double* d_s,
                         int32_t* d_status);
msm_status msm_tram_update(msm_ctx* ctx, int K, int m, const double* d_N, const double* d_tab, const double* d_s,
                           const double* d_v, double* d_f, double* d_g, double* d_err);
msm_status msm_tram_iterations(msm_ctx* ctx, const void* d_u, msm_dtype dtype, int K, int m, int64_t N, int64_t ld,
                               const int64_t* d_offsets, const int64_t* d_unit_ptr, const int32_t* d_unit_state,
                               int64_t units, const double* d_S, const double* d_N, const double* d_col, double* d_f,
                               double* d_v, double* d_work, int n_iterations, int max_workgroups, double* d_logden,
                               double* d_err, int32_t* d_status);
msm_status msm_tram_transition_matrices(msm_ctx* ctx, int K, int m, const double* d_S, const double* d_N,
                                        const double* d_f, const double* d_v, int k, double* d_rowsum, double* d_P);

/* ---- HMM: discrete-output hidden Markov models, Baum-Welch on the device (csrc/hmm.hip) ---------------
 * Written from the published method (Rabiner 1989; the lagged sequences of deeptime's lag_observations).  Parity
 * with deeptime or PyEMMA is NOT pinned; the tests hold the kernels to tests/_hmm_ref.py run in 80-bit floats.
 *
 * n hidden states (1 <= n <= MSM_HMM_MAX_HIDDEN, MSM_ERR_UNSUPPORTED above), k >= 1 symbols, d_A f64 [n, n],
 * d_B f64 [n, k], d_p0 f64 [n].  d_labels int32 [N].  d_seq int64 [Q, 3] holds (start, stride, length): observation
 * t of sequence q is labels[start_q + t stride_q].  Chunk c of a sequence of length T covers the steps
 * t = 1 + cL .. min((c+1)L, T-1), L = MSM_HMM_CHUNK; a sequence of length 1 has none.  d_chunk_ptr int64 [Q + 1] is
 * the prefix sum of the chunk counts and d_chunk_seq int32 [n_chunks] names every chunk's sequence.  A triple or a
 * chunk range that does not describe frames of [0, N) sets MSM_HMM_BAD_TABLE and is not walked.
 *
 * msm_hmm_estep: scaled forward-backward,
 *   alpha^_0 = p0 o b_0 / c_0, alpha^_t = (alpha^_{t-1} A) o b_t / c_t, beta^_{T-1} = 1,
 *   beta^_t = A (b_{t+1} o beta^_{t+1}) / c_{t+1}, gamma_t = alpha^_t o beta^_t.
 *   d_gamma  f64 [N, n] in frame order; only rows of frames in a sequence are written (the caller zeroes it once)
 *   d_C      f64 [n, n] = sum_q sum_t alpha^_t(i) A_ij b_{t+1}(j) beta^_{t+1}(j) / c_{t+1}
 *   d_gamma0 f64 [n] = sum_q gamma_0;  d_logL f64 [Q] = sum_t ln c_t;  d_total f64 [1] = sum_q logL (may be NULL)
 * in three phases: every chunk's product P_c = prod_t A diag(b_t), rescaled by exact powers of two; per sequence
 * the entry vectors a_{c+1} = a_c P_c / sum and exit vectors w_c = P_c w_{c+1} / sum of its chunks; every chunk's
 * replay of alpha^ from a_c (kept in LDS) and walk of beta^ back from w_{c+1}, scaled so that alpha^ . beta^ = 1.
 * The partial C and sum of ln c_t of a sequence's chunks, then the sequences, are added in ascending order: every
 * output has the same bits on every run and for every max_workgroups (0: the default grid).  No fp atomics.
 * A symbol outside [0, k) sets MSM_HMM_BAD_SYMBOL, a sequence of probability 0 sets MSM_HMM_ZERO_PROB; either
 * sequence reports logL = -inf, has zero rows in d_gamma and adds nothing to d_C and d_gamma0.
 * d_work: msm_hmm_workspace_bytes(n, n_chunks, Q, units) bytes (units = 0 where no emission sums are taken).
 *
 * msm_hmm_emissions: E[i, y] = sum of gamma_t(i) over the frames with label y, from msm_group_by_label's
 * d_offsets / d_members.  Unit tables as msm_tram_pass takes them (symbol, segment of 256 member frames):
 * d_unit_ptr int64 [k + 1], d_unit_state int32 [units]; d_part f64 [units, n]; a fold adds the units of a symbol in
 * ascending order.
 *
 * msm_hmm_mstep, one workgroup: B_iy = E_iy / sum_y E_iy; A = the rows of C over their sums, or (reversible) the
 * fixed point msm_reversible_mle documents run on C, checked every iteration, until maxerr or maxiter
 * (<= MSM_HMM_MAX_FIXED_POINT; MSM_HMM_NOT_CONVERGED at maxiter); d_pi f64 [n] = the stationary vector of the new A
 * (the fixed point's x, or the GTH elimination); p0 = gamma0 / Q, or (stationary) pi.  A hidden state without mass
 * keeps its row and sets MSM_HMM_EMPTY_STATE.
 *
 * msm_hmm_iterations: n_iterations of (estep, emissions, mstep) enqueued back to back, nothing read back in between;
 * d_history f64 [n_iterations] receives sum_q logL of every iteration (the likelihood of the parameters the
 * iteration started from).  d_A, d_B, d_p0 are updated in place.
 *
 * msm_hmm_viterbi: the most probable hidden path of every sequence, by the same chunking in the (max, +) semiring on
 * ln A, ln B, ln p0 (taken on the device; ln 0 = -inf).  The chunk products are the kernel of the E-step's products
 * instantiated for (max, +); per sequence delta at every chunk entry, then the boundary states backwards,
 * s_c = argmax_i delta_c(i) + P_c(i, s_{c+1}); every chunk replays from its one-hot entry state with back-pointers
 * in LDS and backtracks from its exit state.  Ties go to the lowest index.  d_path int32 [N] in frame order, -1 for
 * frames in no sequence and for sequences of probability 0 (MSM_HMM_ZERO_PROB) or with a bad symbol; d_logp f64 [Q]
 * (may be NULL) = the path's log-probability as the device added it, -inf for such sequences.
 * d_work: msm_hmm_viterbi_workspace_bytes(n, k, n_chunks, Q) bytes.
 *
 * msm_hmm_plan: read-only; out = {MSM_HMM_CHUNK, padded n, n_chunks, grid of the products and the pass, grid of the
 * boundaries, LDS bytes of the products, of the pass, of an emission unit}. */
#define MSM_HMM_MAX_HIDDEN 16
#define MSM_HMM_CHUNK 64
#define MSM_HMM_MAX_FIXED_POINT 1000000
#define MSM_HMM_BAD_SYMBOL 1
#define MSM_HMM_ZERO_PROB 2
#define MSM_HMM_EMPTY_STATE 4
#define MSM_HMM_BAD_TABLE 8
#define MSM_HMM_NOT_CONVERGED 16
size_t msm_hmm_workspace_bytes(int n, int64_t n_chunks, int Q, int64_t units);
msm_status msm_hmm_plan(msm_ctx* ctx, int n, int64_t n_chunks, int Q, int max_workgroups, int64_t out[8]);
msm_status msm_hmm_estep(msm_ctx* ctx, const int32_t* d_labels, int64_t N, int k, int n, const int64_t* d_seq, int Q,
                         const int64_t* d_chunk_ptr, const int32_t* d_chunk_seq, int64_t n_chunks, const double* d_A,
                         const double* d_B, const double* d_p0, int max_workgroups, void* d_work, double* d_gamma,
                         double* d_C, double* d_gamma0, double* d_logL, double* d_total, int32_t* d_status);
msm_status msm_hmm_emissions(msm_ctx* ctx, const double* d_gamma, int64_t N, int n, int k, const int64_t* d_offsets,
                             const int32_t* d_members, const int64_t* d_unit_ptr, const int32_t* d_unit_state,
                             int64_t units, int max_workgroups, double* d_part, double* d_E);
msm_status msm_hmm_mstep(msm_ctx* ctx, int n, int k, int Q, const double* d_C, const double* d_E,
                         const double* d_gamma0, int reversible, int stationary, int maxiter, double maxerr,
                         double* d_A, double* d_B, double* d_p0, double* d_pi, int32_t* d_status);
size_t msm_hmm_viterbi_workspace_bytes(int n, int k, int64_t n_chunks, int Q);
msm_status msm_hmm_viterbi(msm_ctx* ctx, const int32_t* d_labels, int64_t N, int k, int n, const int64_t* d_seq, int Q,
                           const int64_t* d_chunk_ptr, const int32_t* d_chunk_seq, int64_t n_chunks, const double* d_A,
                           const double* d_B, const double* d_p0, int max_workgroups, void* d_work, int32_t* d_path,
                           double* d_logp, int32_t* d_status);
msm_status msm_hmm_iterations(msm_ctx* ctx, const int32_t* d_labels, int64_t N, int k, int n, const int64_t* d_seq,
                              int Q, const int64_t* d_chunk_ptr, const int32_t* d_chunk_seq, int64_t n_chunks,
                              const int64_t* d_offsets, const int32_t* d_members, const int64_t* d_unit_ptr,
                              const int32_t* d_unit_state, int64_t units, int reversible, int stationary, int maxiter,
                              double maxerr, int n_iterations, int max_workgroups, void* d_work, double* d_A,
                              double* d_B, double* d_p0, double* d_pi, double* d_gamma, double* d_C, double* d_E,
                              double* d_gamma0, double* d_logL, double* d_history, int32_t* d_status);

/* ---- Metadynamics: hills bias, its gradient, the c(t) scan, a device ledger (csrc/metad.hip) ---------
 * Written from Laio & Parrinello, PNAS 99, 12562 (2002), Barducci, Bussi & Parrinello, PRL 100, 020603 (2008) and
 * Tiwary & Parrinello, J. Phys. Chem. B 119, 736 (2015), with the cutoff and the stretched kernel as PLUMED's METAD
 * documents them.  The tests hold the kernels to a numpy restatement of the rule below (tests/_metad_ref.py), run in
 * 80-bit floats.  Everything is fp64.
 *
 * d_hills f64 [H, 2 d + 1]: hill k is the record (centre [d], 1 / sigma [d], height); sigma is per hill, diagonal.
 * h_period f64 [d] or NULL: the period of a periodic CV, 0 for one that is not.  The term of hill k at the point s:
 *     dp_i = s_i - c_i;   periodic:  dp_i -= P_i * rint(dp_i / P_i);   z_i = dp_i * (1 / sigma_i)
 *     dp2  = 0.5 * sum_i z_i^2   (ascending i);   the term and its gradient are 0 where dp2 >= cut  (cut > 0)
 *     term = h * (A * exp(-dp2) + B),   d term / d s_i = -(h * (A * exp(-dp2))) * (z_i * (1 / sigma_i))
 *   MSM_METAD_GAUSSIAN: A = 1, B = 0.  MSM_METAD_STRETCHED: A = 1 / (1 - exp(-cut)), B = -exp(-cut) * A, which
 *   brings the term to 0 at the cutoff (PLUMED's default kernel).
 * msm_metad_bias: d_cv f64 [n, ld], the first d columns of a row are a frame's CVs.  Frame f adds the hills
 *   0 .. count[f] - 1 (d_count int32 [n], clamped to [0, H]; NULL: all H), in ascending hill index, into
 *   d_bias f64 [n] and, where d_grad is not NULL, d_grad f64 [n, ldg] (columns 0 .. d - 1).  H = 0 gives zeros.
 *   A frame with a non-finite CV is NaN in its own outputs and nowhere else.
 *   Launch shape (msm_metad_plan: out = frames per workgroup, hills per tile, grid, LDS bytes): one frame per lane,
 *   MSM_METAD_THREADS frames per workgroup trip in a grid-stride loop (max_workgroups > 0 caps the grid), the hills
 *   staged through LDS in tiles of MSM_METAD_TILE.  A workgroup walks the hills up to the largest count of its
 *   frames.  No lane shares a sum with another: a frame's bits depend on its CVs, its count and the hills alone, not
 *   on the grid, the tile or its neighbours.  No scratch memory.
 * msm_metad_grid_scan: a regular grid of d <= MSM_METAD_GRID_MAX_D CVs, point (i_0, .., i_{d-1}) at
 *   lo_a + i_a * step_a, the last axis fastest, G = prod bins (a periodic axis carries no duplicate end point).
 *   h_checkpoints int32 [M], ascending in [0, H]; a1 >= a2 >= 0.  Every lane keeps V of one grid point in a register
 *   and walks all hills once in order; at checkpoint k_j (V_{k_j}: the first k_j hills) a workgroup forms
 *   (max, sum exp(a V - max)) of its MSM_METAD_SCAN_TILE points for both exponents in a fixed order, and a second
 *   launch merges the tiles in a fixed order (lane l of a wave adds the tiles l, l + 64, .. ascending, then a shuffle
 *   tree):  d_lse f64 [M, 2],  lse[j, e] = log sum_g exp(a_e V_{k_j}(g)).
 *   The maximum is subtracted before every exp, so a V may be of any size.  d_vgrid f64 [G] (may be NULL) receives
 *   V_H.  The tile is fixed, so the bits do not depend on max_workgroups.  A negative, NaN or infinite height is
 *   MSM_ERR_INVALID (the heights are read back before the scan is launched: the call waits for the stream, and is
 *   not for graph capture).
 * msm_metad_append: writes record `index` of a ledger of `capacity` records from h_record f64 [2 d + 1], passed to
 *   the kernel by value: nothing is staged and nothing waits.  d_center (f64 [d], may be NULL) replaces the centre by
 *   CVs that are still on the device; d_v (f64 [1], may be NULL) scales the height by exp(v_scale * d_v[0]): the
 *   well-tempered rule h0 exp(-V(centre) / ((gamma - 1) kT)) with V evaluated by msm_metad_bias just before. */
#define MSM_METAD_MAX_D 8
#define MSM_METAD_GRID_MAX_D 3
#define MSM_METAD_THREADS 256
#define MSM_METAD_TILE 128
#define MSM_METAD_SCAN_TILE 256
#define MSM_METAD_GAUSSIAN 0
#define MSM_METAD_STRETCHED 1
msm_status msm_metad_plan(msm_ctx* ctx, int64_t n, int H, int d, int max_workgroups, int64_t out[4]);
msm_status msm_metad_bias(msm_ctx* ctx, const double* d_cv, int64_t n, int64_t ld, int d, const double* d_hills, int H,
                          const double* h_period, int kernel, double cut, const int32_t* d_count, int max_workgroups,
                          double* d_bias, double* d_grad, int64_t ldg);
msm_status msm_metad_grid_scan(msm_ctx* ctx, const double* d_hills, int H, int d, const double* h_lo,
                               const double* h_step, const int32_t* h_bins, const double* h_period, int kernel,
                               double cut, const int32_t* h_checkpoints, int M, double a1, double a2,
                               int max_workgroups, double* d_lse, double* d_vgrid);
msm_status msm_metad_append(msm_ctx* ctx, double* d_hills, int capacity, int index, int d, const double* h_record,
                            const double* d_center, const double* d_v, double v_scale);

/* ---- OPES: compressed kernels, the journal of their versions, bias and gradient (csrc/opes.hip) -------
 * Written from Invernizzi & Parrinello, J. Phys. Chem. Lett. 11, 2731 (2020) (OPES_METAD).  The definition is this
 * library's own ("OPES"); the tests hold the kernels to tests/_opes_ref.py run in 80-bit floats.  fp64.
 *
 * h_par f64 [MSM_OPES_PARAMS]: kT, p = 1 - 1 / gamma, epsilon, cutoff, compression threshold, fixed_sigma (0 / 1),
 *   period [MSM_METAD_MAX_D] (0: not periodic), sigma0 [MSM_METAD_MAX_D] (read by the on-line deposit only).
 * A kernel is the record (centre [d], sigma [d], height) of 2 d + 1 doubles.  With dp_i the minimum image of
 *   s_i - c_i (dp_i -= P_i * rint(dp_i / P_i)), q = sum_i (dp_i / sigma_i)^2 in ascending i and v = exp(-cutoff^2 / 2):
 *     G(s) = h * (exp(-q / 2) - v) where q < cutoff^2, else 0.
 *   P(s) = sum_live G(s) / W,   V(s) = kT p log(P(s) / Z + epsilon),
 *   dV / ds_i = kT p ((sum_live dG / ds_i / W) / Z) / (P / Z + epsilon);
 *   no deposit yet: V = kT p log(epsilon), formed on the host, and dV = 0.
 * The ledger on the device, all of `capacity` entries: d_live f64 [capacity, 2 d + 1] (the first K slots live),
 *   d_slot_version int32 [capacity] (the version a slot holds), d_journal f64 [capacity, 2 d + 1] (version j is what
 *   deposit j left: the appended or the finally merged kernel), d_death int32 [capacity] (the deposit that removed the
 *   version, INT32_MAX while it lives: after deposits 0 .. c - 1 the live set is {j < c : death_j >= c}),
 *   d_per_deposit f64 [capacity, MSM_OPES_PER_DEPOSIT] = W, Z, neff, K after deposit j, and
 *   d_state f64 [MSM_OPES_STATE] = deposits so far, K, W = sum w, W2 = sum w^2, S = sum_k sum_k' G_k'(c_k), Z,
 *   status bits, cursor.  A fresh state is 0 everywhere except Z = 1.
 * msm_opes_deposit: ONE launch of one wave that consumes up to max_steps of the n_records deposits, from the cursor
 *   in the state on (restart != 0: from record 0); the caller repeats the launch ceil(n_records / max_steps) times
 *   and nothing waits.  d_records f64 [n_records, 2 d + 2] = centre, sigma, height, logweight.  d_cv == NULL: the
 *   records are given and w = exp(logweight).  d_cv f64 [n_records, ld]: deposit r is made at the CVs of row r with
 *   logweight = V(s) / kT of the state so far, w = h = exp(logweight), then W += w, W2 += w^2,
 *   neff = (1 + W)^2 / (1 + W2), and unless fixed_sigma sigma_i = sigma0_i (neff (d + 2) / 4)^(-1 / (d + 4)) and
 *   h *= prod_i sigma0_i / sigma_i; the record made is written to d_records.  Then, both forms alike: the live kernel
 *   k* with the smallest sum_i (dp_i / sigma*_i)^2 (lowest slot on a tie; lanes take slots l, l + 64, .., then a fixed
 *   arg-min tree) takes the kernel in if that value < threshold^2:  h = h1 + h2,  c = c1 + (h2 / h) dp,
 *   sigma^2 = (h1 sigma1^2 + h2 sigma2^2) / h + (h1 h2 / h^2) dp^2  (1: k*, 2: the incoming kernel, dp the minimum
 *   image of c2 - c1), the merged kernel keeps slot k* and is tested against the others again, at most K times; a
 *   chain merge keeps the lower slot and the last live slot fills the higher.  Otherwise the kernel is appended.
 *   S loses the pairs of every kernel removed and gains those of the kernel added (each a sum over the live slots in
 *   the lane order above), Z = S / (W K).  A full ledger (MSM_OPES_FULL), a record with a non-finite centre or
 *   logweight or a sigma or height that is not positive and finite (MSM_OPES_BAD_RECORD) and a state that does not fit
 *   the buffers (MSM_OPES_BAD_STATE) set their bit in the state and consume nothing more: a launch that finds the
 *   status not 0 returns at once, so the ledger stays as the last accepted deposit left it until the caller writes
 *   0 to the status word.
 * msm_opes_bias, journal form (d_death != NULL): d_kernels is the journal of T versions; frame f with count c
 *   (d_count int32 [n], clamped to [0, T]; NULL: T, the final bias) adds the versions j < c <= death_j in ascending j
 *   with 1 / sigma formed once per tile, and reads W, Z of deposit c - 1.  One frame per lane, MSM_METAD_THREADS
 *   frames per workgroup trip, tiles of MSM_METAD_TILE versions; a tile whose versions all died before the smallest
 *   count of the workgroup is skipped unless MSM_OPES_NO_SKIP is set (the bits are the same).  A frame's bits depend
 *   on its CVs, its count and the journal alone.  A frame with a non-finite CV is NaN in its own outputs.  Where
 *   d_state is given, T is lowered to the deposits the device has made (a caller that did not wait cannot know of a
 *   refused deposit): no row is read that was never written.
 *   Live form (d_death == NULL, d_count == NULL): d_kernels is d_live, T its capacity, and K, W, Z are read from
 *   d_state on the device; one wave per frame in the order of the deposit's own V(s) (n = 1 is the MD step).
 * msm_opes_plan: out = frames per workgroup, versions per tile, grid, LDS bytes, threads of the deposit launch,
 *   grid of the live form.  No scratch memory anywhere. */
#define MSM_OPES_PARAMS (6 + 2 * MSM_METAD_MAX_D)
#define MSM_OPES_PAR_KT 0
#define MSM_OPES_PAR_PREFACTOR 1
#define MSM_OPES_PAR_EPSILON 2
#define MSM_OPES_PAR_CUTOFF 3
#define MSM_OPES_PAR_THRESHOLD 4
#define MSM_OPES_PAR_FIXED_SIGMA 5
#define MSM_OPES_PAR_PERIOD 6
#define MSM_OPES_PAR_SIGMA0 (6 + MSM_METAD_MAX_D)
#define MSM_OPES_STATE 8
#define MSM_OPES_STATE_COUNT 0
#define MSM_OPES_STATE_LIVE 1
#define MSM_OPES_STATE_W 2
#define MSM_OPES_STATE_W2 3
#define MSM_OPES_STATE_SUM 4
#define MSM_OPES_STATE_Z 5
#define MSM_OPES_STATE_STATUS 6
#define MSM_OPES_STATE_CURSOR 7
#define MSM_OPES_PER_DEPOSIT 4
#define MSM_OPES_FULL 1
#define MSM_OPES_BAD_RECORD 2
#define MSM_OPES_BAD_STATE 4
#define MSM_OPES_NO_SKIP 1
msm_status msm_opes_plan(msm_ctx* ctx, int64_t n, int T, int d, int max_workgroups, int64_t out[6]);
msm_status msm_opes_deposit(msm_ctx* ctx, int d, const double* h_par, double* d_state, double* d_live,
                            int32_t* d_slot_version, double* d_journal, int32_t* d_death, double* d_per_deposit,
                            int capacity, double* d_records, int n_records, const double* d_cv, int64_t ld,
                            int max_steps, int restart);
msm_status msm_opes_bias(msm_ctx* ctx, const double* d_cv, int64_t n, int64_t ld, int d, const double* h_par,
                         const double* d_kernels, const int32_t* d_death, const double* d_per_deposit, int T,
                         const int32_t* d_count, const double* d_state, int flags, int max_workgroups, double* d_bias,
                         double* d_grad, int64_t ldg);

/* ------------------------------------------------------------------ */
/* exchange steps of the sharded path (RCCL over xGMI)                  */
/* ------------------------------------------------------------------ */

/* One process per GPU, one trajectory shard per process (the reference has no
 * multi-device code: lag pairs never cross a shard -- S/analysis/discretize.py:625-632 segments,
 * S/markov_state_model/_features.py:216-227 per-trajectory frame dropping -- so only the SMALL
 * per-shard results are summed).  The collectives run on the context's stream, in place, on device
 * buffers; librccl is dlopen'ed by the first msm_comm_unique_id / msm_comm_init.
 *
 *   msm_comm_unique_id     rank 0 draws the 128-byte RCCL id; the caller carries it to the other ranks
 *                          (file, environment, any store: pmarlo_amd/dist.py uses a file)
 *   msm_comm_init          collective over `world` processes (ncclCommInitRank)
 *   msm_allreduce_i64      exact integer sum: k-means member sums / counts, transition counts, the
 *                          batched L x k x k lag-scan counts (one call)
 *   msm_allreduce_f64      fp64 sum in RANK ORDER (all-gather + fixed-order add): moment blocks; the same
 *                          bits on every rank and for every algorithm RCCL may choose
 *   msm_allreduce_min_f64  / _max_f64: the fixed-point scale of the Lloyd sums; timing maxima
 *   msm_broadcast          bytes from `root`: the shared shift vector, the initial centres
 *   msm_comm_info          rank, world and the number of collectives issued so far
 *   msm_rcp_f64            dst[i] = 1 / src[i] on the stream (2^-e after the MIN of 2^e: exact) */
typedef struct msm_comm msm_comm;
#define MSM_COMM_ID_BYTES 128
msm_status msm_comm_unique_id(void* out_id, size_t bytes);
msm_status msm_comm_init(msm_ctx* ctx, int rank, int world, const void* id, size_t id_bytes, msm_comm** out);
void msm_comm_destroy(msm_comm* comm);
msm_status msm_comm_info(msm_comm* comm, int* rank, int* world, uint64_t* n_collectives);
msm_status msm_allreduce_i64(msm_comm* comm, int64_t* d_buf, size_t count);
/* the same sum out of place: d_dst = sum over ranks of d_src (the persistent local member sums of the Lloyd passes
 * are reduced straight into the exchange buffer, no copy in front of the collective) */
msm_status msm_allreduce_i64_from(msm_comm* comm, const int64_t* d_src, int64_t* d_dst, size_t count);
msm_status msm_allreduce_f64(msm_comm* comm, double* d_buf, size_t count);
msm_status msm_allreduce_min_f64(msm_comm* comm, double* d_buf, size_t count);
msm_status msm_allreduce_max_f64(msm_comm* comm, double* d_buf, size_t count);
msm_status msm_broadcast(msm_comm* comm, void* d_buf, size_t bytes, int root);
msm_status msm_rcp_f64(msm_ctx* ctx, const double* d_src, size_t n, double* d_dst);

#ifdef __cplusplus
}
#endif
#endif /* MSMHIP_H */
