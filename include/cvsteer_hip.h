/*
 * cvsteer_hip.h -- C ABI of libcvsteer_hip.so: the MI355X (gfx950) engine behind the
 * fa::SteerableFilters / SteerableFiltersG2 / SteerableFiltersG4 classes of
 * headupinclouds/cvsteer.
 *
 * The reference has no FFI layer: its boundary is the C++ class surface
 * (cvsteer/SteerableFilters.h:41-50, SteerableFiltersG2.h:35-67, SteerableFiltersG4.h:35-57)
 * and every arithmetic step is an OpenCV call.  Each entry point below names the reference
 * member function (file:line) whose work it replaces.  The C++ facade in
 * the include/cvsteer/ headers keep the reference's class/method names on top of this ABI;
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *  - every function returns an int status (CVS_OK = 0, negative = error); nothing throws.
 *  - images are `cvs_plane`: row-major f32, `step` bytes between rows (multiple of 4,
 *    >= cols*4), living in host memory (CVS_MEM_HOST) or in the handle's device
 *    (CVS_MEM_DEVICE).  cv::Mat1f maps 1:1: {(float*)m.data, m.rows, m.cols, m.step}.
 *  - a handle owns its state planes (basis, C1..C3, theta, strength) in device memory;
 *    callers own every plane they pass in.  State stays valid until the next cvs_setup.
 *  - a plane may be a region of interest of a larger image (step > row length), and then the rest of that image is the caller's
 *    too: (1) a call writes exactly rows x cols elements of each output plane and not one byte more -- not the padding of a row,
 *    not a row above or below the view; (2) a call never writes to an input (unless the caller passes it as an output too,
 *    where that is allowed); (3) what lies around an input view never changes a result.  This holds for host and device
 *    planes, for 8-bit (CVS_DEPTH_U8) and int32 (CVS_DEPTH_S32) planes, and for the arrays that come with a capacity or a count:
 *    nothing in front of the array and nothing behind its last element is written.
 *  - all device work is enqueued on the handle's HIP stream (default: the null stream;
 *    cvs_set_stream to share e.g. PyTorch's current stream).  Calls with only DEVICE planes
 *    are asynchronous; calls that touch a HOST plane return after the data has landed.
 *  - a handle is not re-entrant; different handles may be used from different threads.
 *  - there is no CPU fallback: without a usable HIP device cvs_create fails with CVS_E_HIP.
 */
#ifndef CVSTEER_HIP_H
#define CVSTEER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): cvs_launch_info carries its size; the placement-search, XCD-weight, store-policy, G4-split and
 * workgroups-per-CU options are gone (9 options left) */
#define CVS_ABI_VERSION 2

/* status codes */
enum {
    CVS_OK = 0,
    CVS_E_BADARG = -1,      /* null pointer, unknown enum, bad index */
    CVS_E_SIZE = -2,        /* empty image, mismatched plane sizes, bad step */
    CVS_E_HIP = -3,         /* HIP runtime error (see cvs_last_error) */
    CVS_E_NOMEM = -4,       /* device or host allocation failed */
    CVS_E_STATE = -5,       /* state not available (no setup yet / orientation not computed) */
    CVS_E_UNSUPPORTED = -6  /* operation the reference does not define for this kind */
};

/* Planes that share memory.  The reference never checks (an output that overlaps its input gives whatever OpenCV's loops
 * happen to produce).  Here it is CVS_E_BADARG, for host planes and device planes alike:
 *   - filter-bank entries (cvs_setup*, cvs_pipeline*, cvs_pyr_down): no output may share a byte with the input image (the
 *     kernels read rows ahead of the rows they write) or with another output;
 *   - per-pixel entries (cvs_steer_*, cvs_mag_phase, cvs_phase_weights, cvs_find, cvs_wrap): an output may BE an input -- same
 *     first pixel, same step; the reference itself calls wrap(m_theta, m_theta) -- but may not overlap one in any other way,
 *     nor another output.
 * Two views with the same step are compared exactly (column ranges of one buffer side by side share nothing and are fine);
 * views with different steps by their address ranges.  f32 planes must be 4-byte aligned. */
enum { CVS_KIND_G2 = 2, CVS_KIND_G4 = 4 };
enum { CVS_MEM_HOST = 0, CVS_MEM_DEVICE = 1 };
/* OR-ed into cvs_plane.mem of an INPUT IMAGE (cvs_setup / cvs_setup_steer / cvs_pipeline[_batch]): `data` points
 * at 8-bit samples (`step` >= cols bytes).  The reference's callers hand 8-bit images to the constructor and let
 * cv::Mat1f(const Mat&) widen them unscaled (test/test.cpp:73,85; example/steer.cpp:73-86); here the 8-bit data
 * crosses PCIe as bytes and is widened on the device. */
enum { CVS_DEPTH_U8 = 0x100 };
/* EXTENSION (contour components): a plane of int32_t (labels); `step` in bytes, a multiple of 4, >= cols * 4.  `data` is the
 * int32_t* cast to float*.  Accepted only where an entry point below says so. */
enum { CVS_DEPTH_S32 = 0x200 };

/* cvs_setup flags */
enum {
    CVS_SETUP_BASIS = 1u,   /* the 7 (G2) / 11 (G4) separable basis planes */
    CVS_SETUP_ORIENT = 2u,  /* + C1,C2,C3, dominant angle, strength (G2 only) */
    CVS_SETUP_FULL = 3u
};

/* options for cvs_set_option.  Process-wide overrides for new handles (A/B aids): the environment variable
 * CVS_OPTS="name=value,..." with autotune=0|1, layout=0|1|2|3, pyr_strip=0|1, batch_ways=N, warm=K (0 = off), wgcap=N (workgroups per CU, 0 = no cap),
 * lit=0|1 (0: never the kernel instances with the default taps compiled in),
 * nt_stores=0|1 (output stores plain / nontemporal instead of by size), verbose=1 (the tuner prints its decisions to stderr),
 * pool_mb=N (state-block cache, default 4096, 0 = off).  Read at every call; results never depend on any of them. */
enum {
    CVS_OPT_ATAN_MODE = 1,   /* 0 = OpenCV-compatible fastAtan2 polynomial (default), 1 = exact atan2f */
    CVS_OPT_STRIP_ROWS = 2,  /* rows per wave strip of the basis kernel (0 = default: chosen by the engine / its tuner) */
    CVS_OPT_FIND_ON = 3,     /* cvs_pipeline: 0 = find*(magnitude, phase) as the reference's callers do
                                (test/test.cpp:88-90), 1 = find*(e, phase) */
    CVS_OPT_G4_EXTENSIONS = 6, /* 0 (default) = G4 exactly as the reference leaves it (no orientation, no e/mag/phase);
                                  1 = EXTENSION beyond the reference: cvs_setup(G4, CVS_SETUP_FULL) fills C1..C3 / theta /
                                  strength from the G4/H4 steering polynomials, cvs_steer_* accept e/mag/phase, and
                                  cvs_pipeline / cvs_pipeline_batch / cvs_batch_run run the caller sequence for G4 */
    CVS_OPT_BLOCK_ORDER = 8, /* order in which the basis kernel's workgroups take their tiles: -1 (default) = the engine's choice
                                (row-major, unless its tuner finds one of the others faster for this shape on the caller's own
                                launches); 0 = row-major; 1000000 = every XCD walks its own range of column blocks;
                                2000000 = row-major with a DYNAMIC TAIL: the last tenth of the tiles is handed out on demand
                                from eight per-XCD queues in device memory (grid = static tiles + 1.25 x the tail tiles), so an
                                XCD that is ahead takes over tiles of the others.  Results do not depend on it. */
    CVS_OPT_PERSIST_STATE = 9, /* cvs_pipeline / cvs_pipeline_batch: 1 (default) = keep basis + orientation planes like the
                                  reference object does; 0 = write the requested outputs only (no state afterwards) */
    CVS_OPT_AUTOTUNE = 12,   /* 1 (default): while a (kind, entry point, shape bucket) is undecided, each call runs one of a few launch
                                configurations, every candidate in sustained turns of 20-100 consecutive calls timed as a whole between
                                two events on the caller's stream (no extra launches, no waiting); the engine keeps a challenger only
                                when its turns are 3 % ahead of the default's, consistently; 0 = always the
                                defaults */
    CVS_OPT_HOST_OVERLAP = 13, /* cvs_setup / cvs_setup_steer / cvs_pipeline with HOST planes on images of 1 Mpix and more:
                                  1 (default) = the image goes up, is filtered and comes down in row bands, all three at once
                                  (full-duplex host link, a second host thread for the downloads); 0 = one after the other */
    CVS_OPT_STATE_LAYOUT = 14  /* how the handle's state planes lie in its block.  1 (default) = ROW-INTERLEAVED: row r of all basis
                                  planes side by side ([row][plane][column]; the five orientation planes likewise, in a group of
                                  their own) -- a launch that writes 7..12 planes then streams ONE linear sweep per group instead of
                                  one stream per plane 64 MiB apart; every plane is still an ordinary strided
                                  image (cvs_state_plane: step = planes x row length).  0 = planar, plane after plane (also what
                                  groups of 2 GiB and more use).  With 1 the engine puts all twelve G2 planes into ONE group for
                                  single-image launches that write the orientation planes too (full setup, caller pipeline: one
                                  write sweep instead of two; cvs_launch_info.state_layout = 2 then) and uses the two groups for
                                  every other launch; 2 = the same, spelled out; 3 = always two groups.
                                  Takes effect at the next cvs_setup*; results do not depend on it.
                                  NOTE: because the grouping may change from one setup to the next, a cvs_state_plane view is
                                  valid only until the handle's next cvs_setup* / cvs_pipeline* call. */
};

/* state planes addressable through cvs_state_plane / cvs_read_state */
enum {
    CVS_PLANE_BASIS0 = 0,    /* + p, p < cvs_num_basis(kind): m_g2a..m_h2d / m_g4a..m_h4f */
    CVS_PLANE_C1 = 32, CVS_PLANE_C2 = 33, CVS_PLANE_C3 = 34,
    CVS_PLANE_THETA = 35,    /* getDominantOrientationAngle()    */
    CVS_PLANE_STRENGTH = 36  /* getDominantOrientationStrength() */
};

typedef struct cvs_plane {
    float* data;
    int32_t rows;
    int32_t cols;
    size_t step;   /* bytes */
    int32_t mem;   /* CVS_MEM_HOST | CVS_MEM_DEVICE */
} cvs_plane;

typedef struct cvs_context* cvs_handle;

/* ---------------- library / host-only helpers (no GPU needed) ---------------- */
int cvs_abi_version(void);
const char* cvs_status_string(int status);
/* number of 1-D tap vectors == number of basis planes: 7 (G2), 11 (G4) */
int cvs_num_basis(int kind);
/* SteerableFilters::create (SteerableFilters.cpp:33-42) applied to the idx-th tap function
 * (SteerableFiltersG2.cpp:35-42 order m_g1,m_g2,m_g3,m_h1..m_h4; SteerableFiltersG4.cpp:34-45
 * order m_g1..m_g5,m_h1..m_h6).  out: 2*width+1 floats. */
int cvs_make_taps(int kind, int idx, int width, float spacing, float* out);
/* which taps build basis plane p: sepFilter2D(image, kx=taps[*kx], ky=taps[*ky])
 * (SteerableFiltersG2.cpp:62-68, SteerableFiltersG4.cpp:69-80) */
int cvs_basis_taps(int kind, int p, int* kx, int* ky);
/* scalar steering weights for theta (SteerableFiltersG2.cpp:140-142, G4.cpp:116-119):
 * out[0..2]=ga,gb,gc out[3..6]=ha..hd (G2) ; out[0..4]=ga..ge out[5..10]=ha..hf (G4) */
int cvs_steer_weights(int kind, float theta, float* out);

/* ---------------- handle ---------------- */
/* SteerableFiltersG2::SteerableFiltersG2 / G4 ctor minus setup (G2.cpp:44-56, G4.cpp:47-63):
 * builds the tap vectors, binds HIP device `device`. */
int cvs_create(int kind, int width, float spacing, int device, cvs_handle* out);
/* ~SteerableFiltersG2/G4.  The handle's state block (its largest allocation) is not freed but parked in a
 * process-wide cache -- the reference's callers build one short-lived object per image (example/steer.cpp:86,
 * test/test.cpp:85), and the next handle on the same device takes the block over instead of allocating.
 * The cache is bounded (CVS_OPTS pool_mb, default 4096; 0 = off). */
int cvs_destroy(cvs_handle h);
/* frees every block held by that cache */
int cvs_release_cached_memory(void);
const char* cvs_last_error(cvs_handle h);
/* Bind the handle to a HIP stream.  The handle's buffers are reused from call to call, so when the stream changes
 * the new stream is made to wait (event, no host sync) for the work already queued on the old one. */
int cvs_set_stream(cvs_handle h, void* hip_stream);
int cvs_set_option(cvs_handle h, int option, int value);
int cvs_get_option(cvs_handle h, int option, int* value);
/* How the handle's last basis launch was configured (launch order, strip height, store policy, state layout: the defaults
 * or what the online tuner kept).  For benchmarks and tests; nothing of this changes results.  The caller sets struct_size =
 * sizeof(cvs_launch_info) before the call; the library fills at most that many bytes (a client built against an older, shorter
 * struct keeps working). */
typedef struct cvs_launch_info {
    uint32_t struct_size;     /* in: sizeof(cvs_launch_info) of the caller */
    int32_t block_order;      /* last basis launch: CVS_OPT_BLOCK_ORDER value in effect */
    int32_t strip_rows;       /* ... output rows per wave strip */
    int32_t nt_stores;        /* ... 1 = streaming (nontemporal) stores */
    int32_t state_layout;     /* layout of the current state block: 0 = planar, 1 = row-interleaved groups (CVS_OPT_STATE_LAYOUT),
                                 2 = row-interleaved with the G2 orientation planes in the basis planes' group (what launches that write them use) */
    int32_t warm;             /* last basis launch: K > 0 = the launch took its image for a NEW one (another pointer than the handle's
                                 previous call) and the waves of its first row bands requested the rest of the image ahead of need,
                                 K bands each (f32 images of 24 MiB and more; not for 8-bit images, frame batches and launches that
                                 also emit a pyramid level); 0 = not */
    int32_t tuning_launches;  /* launches the engine has issued on this handle's stream beyond the caller's own calls: always 0
                                 (configurations are compared on the caller's launches) */
    int32_t tuned;            /* 1 = the configuration above is a challenger the online tuner decided for; 0 = the engine's default */
    int32_t tune_state;       /* the online tuner for this launch's key: 0 = off / not a tunable launch, 1 = still comparing on the
                                 caller's launches, 2 = decided */
    int32_t wg_per_cu;        /* last basis launch: workgroups per CU it was held to (single G2 images of 2 Mpix and more: three or four
                                 instead of the six the registers allow -- fewer write fronts); 0 = no cap */
    int32_t literal_taps;     /* last basis launch: 1 = it ran a kernel instance with the reference's default G2 / H2 taps compiled in as literal
                                 operands (the caller-pipeline variants of a handle made with width 4, spacing 0.67f: same values, cheaper
                                 instruction issue); 0 = taps from the kernel arguments (any other handle or launch) */
    int32_t u8_out;           /* last cvs_pipeline / cvs_pipeline_batch call: how it made its 8-bit outputs.  0 = it had none; 1 = quantised in
                                 the filter launch (gain); 2 = min / max reduced in the filter launch, then one quantise launch (normalise);
                                 3 = composed: f32 maps into the handle's scratch, then the cvs_normalize_u8 / cvs_convert_u8 kernels */
} cvs_launch_info;
int cvs_get_launch_info(cvs_handle h, cvs_launch_info* out);
/* the handle's idx-th tap vector (m_g1.. members), 2*width+1 floats */
int cvs_taps(cvs_handle h, int idx, float* out);
int cvs_kind(cvs_handle h, int* kind, int* width, float* spacing);
/* size of the image of the last cvs_setup (0,0 before) */
int cvs_shape(cvs_handle h, int* rows, int* cols);
int cvs_sync(cvs_handle h);

/* ---------------- the hot path ---------------- */
/* SteerableFiltersG2::setup (G2.cpp:60-100) / SteerableFiltersG4::setup (G4.cpp:67-81).
 * One fused kernel: the image is read once; the row pass, the column pass and (with
 * CVS_SETUP_ORIENT) the C1..C3 / cartToPolar / wrap / *0.5 steps run in registers. */
int cvs_setup(cvs_handle h, const cvs_plane* image, unsigned flags);

/* setup + steer(float theta, g, hq) in the same kernel launch: G2.cpp:60-100 followed by
 * G2.cpp:137-145 (G4.cpp:67-81 + G4.cpp:114-122).  This is the headline "filter+steer" unit. */
int cvs_setup_steer(cvs_handle h, const cvs_plane* image, unsigned flags, float theta,
                    const cvs_plane* g, const cvs_plane* hq);

/* cvs_setup restricted to the output rows [row_lo, row_hi) of the image: the band one GPU takes when a single large
 * image (a pyramid level, BASELINE config 3) is split over several GPUs.  The whole image must be
 * present (the rows around the band are read, the image borders reflect as usual).  Values inside the band are
 * bit-identical to those of a whole-image cvs_setup with the same flags.  Images that take the generic path (non-default
 * taps, tiny images) are filtered whole.
 * ROWS OUTSIDE THE BAND keep, bit for bit, what they held -- so that bands add up to a whole image -- when the handle's
 * previous state-establishing call was a cvs_setup / cvs_setup_steer / cvs_setup_pyr / cvs_setup_rows of an image of the
 * same size, with the same flags, and CVS_OPT_STATE_LAYOUT has not been changed since.  After anything else (a fresh
 * handle, another size, other flags, a cvs_pipeline* call, a changed layout option) the engine may lay the planes out
 * anew for this call (CVS_OPT_STATE_LAYOUT: the grouping follows the flags), and the rows outside the band are
 * UNSPECIFIED until bands or a whole-image call have written them; the rows of the band are valid in every case.
 * The state flags afterwards are those of this call's flags (a basis-only band leaves no orientation state); the handle
 * holds one frame, frame 0 selected. */
int cvs_setup_rows(cvs_handle h, const cvs_plane* image, unsigned flags, int row_lo, int row_hi);

/* device view of a state plane (zero copy; valid until the handle's next cvs_setup* / cvs_pipeline* call: the engine may
 * re-lay the planes between calls, see CVS_OPT_STATE_LAYOUT) */
int cvs_state_plane(cvs_handle h, int which, cvs_plane* view);
/* copy a state plane out (getDominantOrientationAngle()/Strength() getters, G2.h:40-41,
 * and the protected m_g2a.. members for tests) */
int cvs_read_state(cvs_handle h, int which, const cvs_plane* dst);

/* steer(float theta, g2, h2) G2.cpp:137-145 / G4.cpp:114-122; with e, mag, phase non-NULL:
 * steer(float theta, g2, h2, e, magnitude, phase) G2.cpp:157-165.  G4: e/mag/phase must be NULL. */
int cvs_steer_scalar(cvs_handle h, float theta, const cvs_plane* g, const cvs_plane* hq,
                     const cvs_plane* e, const cvs_plane* mag, const cvs_plane* phase);
/* steer(const Mat1f& theta, ...) G2.cpp:147-155, :167-177 / G4.cpp:92-112.
 * theta == NULL steers at the handle's own dominant-orientation plane (what both reference
 * callers do: test/test.cpp:86, example/steer.cpp:87). */
int cvs_steer_map(cvs_handle h, const cvs_plane* theta, const cvs_plane* g, const cvs_plane* hq,
                  const cvs_plane* e, const cvs_plane* mag, const cvs_plane* phase);
/* steer(float theta_k, g, h[, e, magnitude, phase]) -- SteerableFiltersG2.cpp:137-145, :157-165 / SteerableFiltersG4.cpp:114-122 --
 * for k = 0 .. n-1 in one pass over the handle's state planes (each basis plane read once per call, not once per angle).
 * EXTENSION beyond the reference, which steers one angle per call.  thetas: n host floats.  outs: a flat array of n*5 planes,
 * angle-major, {g, h, e, magnitude, phase} for each angle (the convention of cvs_pipeline_batch); an entry with data == NULL is
 * not written.  Every written plane equals, bit for bit, what cvs_steer_scalar(h, thetas[k], ...) writes on the same handle.
 * Unlike cvs_steer_scalar, g and h are not required: any non-empty set of kinds may be asked for (e alone is G2 oriented energy
 * at n angles from C1..C3), but the same set for every angle (CVS_E_BADARG otherwise).  f32 planes only; no two planes may share
 * memory; every plane has the handle's image size (CVS_E_SIZE).  e needs orientation state (CVS_E_STATE); G4 e / magnitude / phase
 * need CVS_OPT_G4_EXTENSIONS (CVS_E_UNSUPPORTED).  Addresses the frame chosen by cvs_select_frame.  Device planes where each
 * kind's n planes share a step and lie at a constant distance from one another (a [n][rows][cols] block, or rows interleaved
 * [rows][n][cols]) take one kernel launch per 32 angles, asynchronous on the handle's stream; any other placement (separate
 * allocations, host planes) runs angle by angle with the same values, and returns after the data has landed when a plane is a
 * host plane. */
int cvs_steer_bank(cvs_handle h, const float* thetas, int n, const cvs_plane* outs);
/* steer(const cv::Point& p, theta, g2, h2, e, magnitude, phase) G2.cpp:115-134 (p.x=col, p.y=row).
 * out = {g2, h2, e, magnitude, phase}; e is NaN when orientation state is absent. */
int cvs_steer_point(cvs_handle h, int x, int y, float theta, float out[5]);

/* ---- EXTENSION beyond the reference: orientation peaks -- every local orientation of a pixel, from one read of the basis planes ----
 * The oriented energy E(theta) = g(theta)^2 + h(theta)^2 of the handle's quadrature pair is sampled at K angles per pixel, its circular
 * local maxima are found, refined by a parabola through three samples, and the M strongest are written: the arms of a crossing, a corner
 * or a T, which the single dominant angle of C1..C3 cannot hold.  Reads the basis planes of the frame chosen by cvs_select_frame
 * (CVS_E_STATE without basis state); needs no orientation state and no CVS_OPT_G4_EXTENSIONS; G2 and G4 handles, every state layout,
 * and the state a cvs_pipeline* call left behind.
 * Geometry: theta is the reference's steering angle.  The direction ACROSS the structure, in (column, row) steps, is (cos theta,
 * -sin theta) -- the convention of cvs_nonmax --, so a straight ridge or edge of direction phi peaks at phi + pi/2 (mod pi).
 * Contract, per pixel; every operation is an f32 operation that rounds on its own, the division is correctly rounded:
 *  1. theta_k = (float)((double)k * pi / K), k = 0 .. K-1; (g_k, h_k) are bit for bit what cvs_steer_scalar(h, theta_k, ...) writes.
 *  2. e_k = g_k*g_k + h_k*h_k.
 *  3. emax / emin = the largest / smallest e_k.
 *  4. A pixel with an e_k that is not finite has no peaks; nor has one unless emax - emin > min_contrast * emax.
 *  5. k is a candidate when e_k > e_(k-1) && e_k >= e_(k+1), indices mod K (the plateau rule of cvs_nonmax: one sample of a two-sample
 *     plateau survives), and e_k > min_energy and e_k >= min_ratio * emax.
 *  6. Candidates are ordered by e_k descending, ties by smaller k; the first M are kept.
 *  7. count = min(number of candidates, M).
 *  8. For a kept k, with p = e_(k-1), c = e_k, n = e_(k+1):  num = p - n;  den = (p - 2c) + n;  d = den < 0 ? (0.5*num) / den : 0, then
 *     d = min(max(d, -0.5), 0.5);  angle = ((float)k + d) * (float)(pi / K), plus (float)pi if it is below 0, then minus (float)pi if it is
 *     not below (float)pi -- so angle lies in [0, (float)pi);  energy = c - (0.25*num)*d.
 *  9. Slots from count upward store angle -1.0f and energy 0.0f.
 * angles / energies: NULL, or max_peaks f32 planes each, slot 0 = the strongest peak; count: NULL, or one CVS_DEPTH_U8 plane.  Any
 * non-empty subset may be asked for, and each plane written holds the values of the full call.
 * CVS_E_BADARG: cfg NULL, a struct_size that is not sizeof(cvs_peaks_cfg), n_angles outside 4 .. 32, max_peaks outside 1 ..
 * CVS_PEAKS_MAX, a threshold that is NaN, min_ratio or min_contrast outside [0, 1], all three outputs NULL, a plane of the wrong depth,
 * an output that overlaps another output or a state plane of the selected frame.  A plane of another size than the handle's image:
 * CVS_E_SIZE.  Nothing is written when an argument is refused.
 * Host and device planes, any row step.  Device planes whose slots share a step and follow one another at a constant distance (a
 * [max_peaks][rows][cols] block) take ONE kernel launch, asynchronous on the handle's stream and capturable; nothing
 * is read back.  Host planes, and device planes placed otherwise, are written through the handle's staging arena by the same launch
 * (CVS_E_UNSUPPORTED while the stream is being captured); with a host plane the call returns after the data has landed. */
#define CVS_PEAKS_MAX 4
typedef struct cvs_peaks_cfg {
    unsigned struct_size;   /* sizeof(cvs_peaks_cfg) */
    int n_angles;           /* K, 4 .. 32 */
    int max_peaks;          /* M, 1 .. CVS_PEAKS_MAX */
    float min_energy;       /* a peak needs e_k >  min_energy */
    float min_ratio;        /* ... and e_k >= min_ratio * emax            (0 .. 1) */
    float min_contrast;     /* a pixel has peaks only if emax - emin > min_contrast * emax   (0 .. 1) */
} cvs_peaks_cfg;
int cvs_orientation_peaks(cvs_handle h, const cvs_peaks_cfg* cfg,
                          const cvs_plane* angles,    /* NULL, or M f32 planes: slot 0 = strongest */
                          const cvs_plane* energies,  /* NULL, or M f32 planes */
                          const cvs_plane* count);    /* NULL, or one CVS_DEPTH_U8 plane */

/* computeMagnitudeAndPhase G2.cpp:107-112 (cartToPolar, wrap, patchNaNs) */
int cvs_mag_phase(cvs_handle h, const cvs_plane* g, const cvs_plane* hq,
                  const cvs_plane* mag, const cvs_plane* phase);
/* SteerableFilters::wrap, SteerableFilters.cpp:46-51: out = angle > pi ? angle - 2pi : angle */
int cvs_wrap(cvs_handle h, const cvs_plane* angle, const cvs_plane* out);
/* static phaseWeights G2.cpp:179-186 (k accepted and ignored, like the reference) */
int cvs_phase_weights(cvs_handle h, const cvs_plane* phase, const cvs_plane* lambda,
                      float phi, int signum, float k);
/* findEdges / findDarkLines / findBrightLines G2.cpp:194-212 in one pass; any output may be NULL */
int cvs_find(cvs_handle h, const cvs_plane* e, const cvs_plane* phase,
             const cvs_plane* edges, const cvs_plane* dark, const cvs_plane* bright);

/* EXTENSION beyond the reference: thin n maps (1..3, e.g. edges / dark / bright) to the local maxima of each map across the
 * orientation theta.  theta == NULL: the handle's own CVS_PLANE_THETA of the frame chosen by cvs_select_frame (CVS_E_STATE
 * without orientation state).  in / out: n f32 planes each, all of the handle's image size.
 * Contract: (c, s) = cos / sin(theta) (the ~1-ulp polynomial of the steer kernels); the direction across the contour, in (column,
 * row) steps, is (c, -s).  With ax = |c|, ay = |s|, sx = c >= 0 ? +1 : -1, sy = s >= 0 ? -1 : +1: if ax >= ay, w = ay / ax and the
 * forward sample is (1-w)*m[r][x+sx] + w*m[r+sy][x+sx]; otherwise w = ax / ay and it is (1-w)*m[r+sy][x] + w*m[r+sy][x+sx]; the
 * backward sample negates both steps.  Every product and sum rounds on its own, the division is correctly rounded.  A pixel is
 * kept when m > backward && m >= forward (one pixel of a two-pixel plateau survives) and then stores m bit for bit; every other
 * pixel -- NaN in m, theta or a sample included -- stores 0.0f.  Neighbours outside the image read as 0.0f.
 * n outside 1..3, or an output that overlaps an input (an output may not be an input either) or another output: CVS_E_BADARG;
 * a plane of another size: CVS_E_SIZE; G4 with theta == NULL needs orientation state (CVS_OPT_G4_EXTENSIONS).  Host and device
 * planes; one kernel launch for all n maps, asynchronous on the handle's stream and capturable (device planes). */
int cvs_nonmax(cvs_handle h, const cvs_plane* theta, int n, const cvs_plane* in, const cvs_plane* out);
/* EXTENSION: 8-connected hysteresis on n planes.  A pixel is strong if v > high, weak if low < v <= high; the output is 255 for
 * strong pixels and for weak pixels 8-connected through weak pixels to a strong one, 0 elsewhere (NaN: never kept).
 * out: CVS_DEPTH_U8 planes (bytes) or f32 planes (0.0f / 255.0f, for the facade).  passes (may be NULL): propagation passes run.
 * Synchronises the handle's stream; CVS_E_UNSUPPORTED while the stream is being captured.
 * The result is the unique fixed point of the promotion, whatever the schedule.  low > high, a NaN threshold, n < 1, outputs of
 * mixed depth or any overlap of an output with an input or another output: CVS_E_BADARG; a plane of another size than the
 * handle's image: CVS_E_SIZE.  Nothing is written when an argument is rejected. */
int cvs_hysteresis(cvs_handle h, int n, const cvs_plane* in, float low, float high, const cvs_plane* out, int* passes);

/* ---- EXTENSION beyond the reference: contour components -- label, measure, prune and list linked contours ----
 * Four calls on planes of the handle's image size (CVS_E_SIZE otherwise; CVS_E_STATE before the first setup), host or device,
 * pitched or dense, on the handle's stream; no handle state is read.  Each reads a result back: like cvs_hysteresis they
 * synchronise the handle's stream and return CVS_E_UNSUPPORTED while it is being captured.  Nothing is written when an argument is
 * rejected.  Every launch sequence is fixed by the image size alone, and every result is a function of the inputs alone (integer
 * arithmetic and copies only), bit for bit.
 * FOREGROUND of a mask plane: an f32 pixel iff v > 0.0f (NaN, zeros and negatives are background, so the outputs of cvs_hysteresis
 * and of cvs_nonmax are masks as they stand); a CVS_DEPTH_U8 pixel iff the byte is non-zero. */

/* EXTENSION: 8-connected components of `mask` into the CVS_DEPTH_S32 plane `labels`: 0 for background, components numbered
 * 1 .. count in raster order of their first pixel (smallest row * cols + col).  count may be NULL.  labels not S32, or overlapping
 * mask: CVS_E_BADARG; rows * cols > 2^31 - 2: CVS_E_SIZE. */
int cvs_label(cvs_handle h, const cvs_plane* mask, const cvs_plane* labels, int* count);

typedef struct cvs_component {     /* 40 bytes, all fields 4 bytes */
    int32_t area;                  /* pixels */
    int32_t x0, y0, x1, y1;        /* bounding box, inclusive (x = column, y = row) */
    int32_t first_x, first_y;      /* first pixel in raster order */
    int32_t peak_x, peak_y;        /* where `peak` is attained; the first such pixel in raster order; -1, -1 if none */
    float peak;                    /* largest non-NaN weight over the component (-0.0f < +0.0f); -INFINITY if none */
} cvs_component;
/* EXTENSION: table[k - 1] describes label k of the CVS_DEPTH_S32 plane `labels`; `table` holds count entries in host or device
 * memory (table_mem = CVS_MEM_HOST / CVS_MEM_DEVICE).  weight: an f32 plane (typically the thinned map the mask came from), or NULL:
 * then no peak.  Pixels whose label lies outside 1 .. count are skipped; a label in 1 .. count that no pixel carries gets area 0
 * and every position -1 (x0 = y0 = x1 = y1 = first_x = first_y = -1).  count == 0: nothing to do; count < 0, a NULL
 * table with count > 0, labels not S32, weight not f32: CVS_E_BADARG. */
int cvs_component_stats(cvs_handle h, const cvs_plane* labels, int count, const cvs_plane* weight,
                        cvs_component* table, int table_mem);

/* EXTENSION: for each of n >= 1 masks: label it, measure it, and write 255 to the pixels of every component with area >= min_area
 * and (when weight != NULL) peak >= min_peak, 0 elsewhere.  out: all CVS_DEPTH_U8 or all f32 (0.0f / 255.0f), as in cvs_hysteresis.
 * weight: NULL or n f32 planes.  kept (may be NULL) receives n ints: components kept per plane.  min_area < 0, NaN min_peak, outputs
 * of mixed depth, any overlap of an output with an input or another output: CVS_E_BADARG. */
int cvs_contour_prune(cvs_handle h, int n, const cvs_plane* mask, const cvs_plane* weight, int min_area,
                      float min_peak, const cvs_plane* out, int* kept);

/* EXTENSION: (x, y, label) int32 triples of all pixels of the CVS_DEPTH_S32 plane `labels` with label != 0, in raster order, into
 * `points` (room for `capacity` triples; points_mem = CVS_MEM_HOST / CVS_MEM_DEVICE).  *n_points (required) is always set to the
 * number of such pixels; when it exceeds capacity the call returns CVS_E_SIZE and writes no triple (capacity = 0, points = NULL
 * sizes the buffer). */
int cvs_contour_points(cvs_handle h, const cvs_plane* labels, int32_t* points, int capacity, int points_mem,
                       int* n_points);

/* EXTENSION: the linked contours of `mask` as ORDERED chains of pixels, cut at junctions and free ends, in a canonical order that
 * depends on the mask alone (integer arithmetic only: bit for bit).  With lin(p) = row * cols + col:
 * LINKS.  Two foreground pixels are linked iff they are 4-adjacent, or they are diagonally adjacent and neither of the two pixels
 * 4-adjacent to both is foreground (the redundant diagonal of a staircase corner is no link).  A pixel has at most 4 links, and the
 * connected components of the links are the 8-connected components of the mask.
 * NODES.  deg(p) = number of links of p; pixels with deg != 2 are nodes: 0 isolated, 1 a free end, >= 3 a junction.
 * CHAINS.  Every link belongs to exactly one chain.  OPEN: a maximal sequence p0 .. pk, k >= 1, of consecutively linked pixels that
 * uses no link twice, with p1 .. p(k-1) of degree 2 and p0, pk nodes (p0 == pk for a loop that leaves and re-enters a junction; a
 * junction appears in each of its chains).  CLOSED: a component whose pixels all have degree 2 is one cycle, listed once from its
 * pixel of smallest lin without repeating that pixel at the end, flag CVS_CHAIN_CLOSED.  ISOLATED: a pixel of degree 0 is a chain of
 * one point.
 * DIRECTION.  An open chain is listed in the direction whose first step (lin(p0), lin(p1)) is lexicographically smaller than the
 * other direction's first step (lin(pk), lin(p(k-1))) -- the two are never equal; a closed chain goes from its smallest pixel
 * towards the smaller of that pixel's two neighbours.
 * ORDER.  Chains are sorted ascending by (lin(p0), lin(p1)), lin(p1) = -1 for an isolated pixel; points are stored chain after
 * chain, so chains[c].start is the running sum of the lengths.  CVS_CHAIN_HEAD_JUNCTION iff deg(p0) >= 3, CVS_CHAIN_TAIL_JUNCTION iff
 * deg(pk) >= 3; neither is ever set on a closed or isolated chain.
 * points: room for point_capacity (x, y) int32 pairs; chains: room for chain_capacity entries; both in host or both in device memory
 * (mem = CVS_MEM_HOST / CVS_MEM_DEVICE).  *n_points and *n_chains (both required) are always set; when either exceeds its capacity
 * the call returns CVS_E_SIZE and writes no point and no chain (points = NULL, chains = NULL with both capacities 0 sizes the
 * buffers).  Always n_points <= 4 * foreground pixels.  The counts follow from degrees and components alone -- open chains = half
 * the sum of the degrees of the nodes, closed chains = components without a node, points = links + open chains + isolated pixels --
 * so the sizing call orders nothing.  A NULL array with a capacity > 0, or a negative capacity: CVS_E_BADARG.
 * Foreground as in cvs_label; f32 or CVS_DEPTH_U8 masks, host or device, pitched or dense.  Like the component calls: synchronises
 * the handle's stream, CVS_E_UNSUPPORTED while it is being captured, CVS_E_STATE before the first setup, CVS_E_SIZE for a plane of
 * another size or for rows * cols > 2^28; nothing is written when an argument is rejected.  The launch sequence depends on the image
 * size and on ceil(log2) of the number of directed links (read back), never on the length or winding of a contour.  Device memory:
 * 10 bytes per pixel and 24 bytes per directed link of handle scratch. */
typedef struct cvs_chain {   /* 16 bytes */
    int32_t start;           /* index of the chain's first point in `points` */
    int32_t length;          /* number of points, >= 1 */
    int32_t flags;           /* CVS_CHAIN_CLOSED = 1, CVS_CHAIN_HEAD_JUNCTION = 2, CVS_CHAIN_TAIL_JUNCTION = 4 */
    int32_t reserved;        /* 0 */
} cvs_chain;
enum { CVS_CHAIN_CLOSED = 1, CVS_CHAIN_HEAD_JUNCTION = 2, CVS_CHAIN_TAIL_JUNCTION = 4 };
int cvs_contour_chains(cvs_handle h, const cvs_plane* mask,
                       int32_t* points, int point_capacity,     /* (x, y) int32 pairs */
                       cvs_chain* chains, int chain_capacity,
                       int mem,                                 /* CVS_MEM_HOST / CVS_MEM_DEVICE, both arrays */
                       int* n_points, int* n_chains);           /* both required, always set */

/* EXTENSION: Ramer-Douglas-Peucker simplification of all chains of a chain table at once: every chain becomes the polyline of its
 * KEPT points.  Needs no image size (any handle, before or after a setup): the handle supplies the stream and the scratch.
 * VIRTUAL LIST.  For chain c with points P[0 .. L), Q = P; for a chain with CVS_CHAIN_CLOSED, Q = P followed by P[0] again, n = L + 1
 * (the repeated point is virtual and never emitted).  Q[0] and Q[n-1] are kept.  L <= 2: every point is kept.
 * SPLIT RULE.  A segment (lo, hi) with hi - lo >= 2, a = Q[lo], b = Q[hi]: for every interior i,
 *   v(i) = |(bx-ax)*(Q[i].y-ay) - (by-ay)*(Q[i].x-ax)| if a != b, else v(i) = (Q[i].x-ax)^2 + (Q[i].y-ay)^2,
 * both int64 and exact for |x|, |y| < 2^28.  m = the SMALLEST i with the largest v.  The test, in IEEE double with one rounding per
 * operation, is num > e2 * den with e2 = (double)eps * (double)eps (exact); for a != b: num = (double)v(m) * (double)v(m) and
 * den = (double)(dx*dx + dy*dy), the sum in int64; for a == b: num = (double)v(m), den = 1.0.  If it holds, Q[m] is kept and (lo, m),
 * (m, hi) are split in turn; otherwise nothing between lo and hi is kept.  The a == b rule is what serves closed chains and open loops
 * that leave and re-enter a junction (p0 == pk).  The kept set does not depend on the order in which segments are visited, and the
 * result is a function of the inputs alone, bit for bit.
 * OUTPUT.  Polyline c = the kept points of chain c in chain order, polylines[c] = (start, length, flags of chains[c], 0) with start
 * the running sum of the lengths; vertices: (x, y) pairs; index (may be NULL): index[k] = position in `points` of vertex k.  Always
 * n_vertices <= n_points, so a caller may allocate n_points vertices and call once.
 * points, chains, vertices, index and polylines are all in host or all in device memory (mem).  *n_vertices (required) is set by every
 * call that gets as far as counting (CVS_OK and CVS_E_SIZE): when it exceeds vertex_capacity the call returns CVS_E_SIZE and writes no
 * vertex, no index and no table entry (vertices = NULL with capacity 0 is the sizing call; polylines may be NULL then and when
 * n_chains == 0).  CVS_E_BADARG, nothing written and *n_vertices untouched: eps NaN or negative (+INFINITY is valid and keeps only the
 * end points), a negative count or capacity, a required array missing, mem invalid, a pointer not aligned to 4 bytes, and a HOST table
 * with an entry that violates start >= 0, length >= 1, start + length <= n_points.  A DEVICE table is trusted for its meaning, but the
 * kernels treat an entry that fails those three conditions as an empty chain (length 0 in the output), so no load or store ever
 * leaves the arrays; coordinates are never used as addresses.  Coordinates outside +-2^28 give unspecified vertices and no fault;
 * n_points > 2^30: CVS_E_SIZE.  Reads one count back: synchronises the handle's stream, CVS_E_UNSUPPORTED while it is being captured.
 * The launch sequence (seven launches) depends on (n_points, n_chains) alone, never on the length or winding of a contour: chains of
 * up to 256 points are carried by one wave each, longer ones by one 256-lane workgroup each.  Device memory: 1 byte per point and
 * 4 bytes per chain of handle scratch (plus 4 bytes per 1024 chains, plus the staged arrays of a host call). */
int cvs_chain_polylines(cvs_handle h,
                        const int32_t* points, int n_points,        /* (x, y) pairs, as cvs_contour_chains writes them */
                        const cvs_chain* chains, int n_chains,      /* chain c = points[start .. start + length) */
                        float eps,
                        int32_t* vertices, int vertex_capacity,     /* (x, y) pairs of the kept points */
                        int32_t* index,                             /* NULL, or vertex_capacity ints: position of each vertex in `points` */
                        cvs_chain* polylines,                       /* NULL only when n_chains == 0 or sizing; else n_chains entries */
                        int mem,                                    /* CVS_MEM_HOST / CVS_MEM_DEVICE: all five arrays */
                        int* n_vertices);                           /* required, always set */

/* ---- EXTENSION beyond the reference: contour edgels -- the sub-pixel position of every chain point, and measures per chain ----
 * Neither call reads anything back: with device arrays (and device planes) each queues its launches on the handle's stream and returns, and
 * both may be captured.  With host arrays the arrays are staged in handle scratch (grown only, freed by cvs_destroy), the call synchronises
 * the stream, and it returns CVS_E_UNSUPPORTED while the stream is being captured.  Nothing is written when an argument is rejected.
 * Sub-pixel polyline vertices need no call of their own: they are xy[index[k]], with the index cvs_chain_polylines returns. */

/* EXTENSION: refine the points (x, y) of a point list -- as cvs_contour_chains writes them -- to the sub-pixel position of the contour and
 * its strength there.  map: an f32 plane of the handle's image size, host or device, pitched or dense.  It is the UN-THINNED response the
 * points were found in (e.g. the edges / dark / bright output of cvs_pipeline, the input of cvs_nonmax): in a thinned map the neighbours of
 * a kept pixel are 0 and the refinement means nothing.  theta: as in cvs_nonmax; NULL = the handle's own CVS_PLANE_THETA of the frame
 * chosen by cvs_select_frame (CVS_E_STATE without orientation state).
 * Contract, per point: m = map[y][x]; (c, s), ax, ay, sx, sy, the major axis, w and the forward / backward samples vf / vb are those of
 * the cvs_nonmax contract -- same operations, same rounding, neighbours outside the image read as 0.0f.  a = m - vb, b = m - vf.  If
 * a > 0 && b >= 0 (the keep test of cvs_nonmax; false for NaN) then t = 0.5f * ((a - b) / (a + b)), every operation rounded on its own,
 * the division correctly rounded -- rounding is monotone, so |t| <= 0.5 without a clamp.  Position: if ax >= ay,
 * xs = (float)x + sx * t and ys = (float)y + sy * (t * w); otherwise xs = (float)x + sx * (t * w) and ys = (float)y + sy * t (sx, sy are
 * +-1: the sign flips are exact).  strength = m + 0.25f * ((a - b) * t): the vertex of the parabola through (vb, m, vf).  Where the test
 * fails -- NaN in m, theta or a sample included -- t = 0, the position is the pixel centre ((float)x, (float)y) and strength is m bit for
 * bit (no product with a NaN sample or weight is formed).
 * xy receives n_points (xs, ys) pairs, strength (may be NULL) n_points floats; points, xy and strength are all in host or all in device
 * memory (mem).  Coordinates are addresses here: the kernel compares them with cols / rows before any load, and a point outside the image
 * stores NaN in xs, ys and strength without the map being read for it; a HOST points array with such a point is refused with
 * CVS_E_BADARG before anything is queued.
 * n_points == 0: CVS_OK, nothing queued.  CVS_E_BADARG: a negative n_points, points or xy NULL with n_points > 0, a pointer not aligned to
 * 4 bytes, an invalid mem, xy or strength overlapping points, map, theta or each other; CVS_E_SIZE: a plane of another size than the
 * handle's image, n_points > 2^30; CVS_E_STATE: no image size yet.  One kernel launch, one lane per point. */
int cvs_chain_refine(cvs_handle h, const cvs_plane* map, const cvs_plane* theta,
                     const int32_t* points, int n_points,   /* (x, y) pairs */
                     float* xy,                              /* n_points (xs, ys) pairs */
                     float* strength,                        /* NULL, or n_points floats */
                     int mem);                               /* CVS_MEM_HOST / CVS_MEM_DEVICE: the three arrays */

/* EXTENSION: table[c] measures chain c of a chain table.  Needs no image size (any handle, before or after a setup).
 * STEPS.  Step i of a chain of L points goes from point i to point i + 1, i < L - 1; a chain with CVS_CHAIN_CLOSED has one more, from
 * its last point to its first.  With (dx, dy) the integer step: |dx| + |dy| == 1 is axial, |dx| == |dy| == 1 diagonal, anything else
 * `other` (always 0 for a table of cvs_contour_chains).  length = the sum over the steps of sqrt(dx * dx + dy * dy) in double, each
 * operation rounded on its own, with dx, dy the differences of the (xs, ys) pairs of `xy` widened to double when xy != NULL, of the
 * integer points otherwise.
 * STRENGTHS.  peak / weakest: the largest / smallest strength of the chain that is not NaN (-INFINITY / +INFINITY if there is none);
 * peak_index: the position in `points` of the first point whose strength equals peak (-1 if none); sum: the IEEE double sum of the
 * chain's strengths (a NaN propagates).  strength == NULL: peak_index -1, peak -INFINITY, weakest +INFINITY, sum 0.
 * The order of the additions of sum and length is fixed by the chain's own length and flags (a lane adds every 64th or 256th term in
 * ascending order, the lanes are combined by a butterfly): the same call twice gives the same bits.  No floating-point atomic is used.
 * points, chains, xy, strength and table are all in host or all in device memory (mem).  A HOST table with an entry that violates
 * start >= 0, length >= 1, start + length <= n_points: CVS_E_BADARG.  On the device such an entry yields an all-zero record with
 * peak_index -1, and no load leaves the arrays; coordinates are never used as addresses.  CVS_E_BADARG as well: a negative count, a
 * required array missing, an invalid mem, a pointer not aligned to 4 bytes, a table that overlaps an input; n_points > 2^30: CVS_E_SIZE.
 * n_chains == 0: CVS_OK, nothing queued.  Two launches for any table -- one wave per chain of up to 256 points, one 256-lane workgroup per
 * longer chain -- so the launch sequence depends on (n_points, n_chains) alone. */
typedef struct cvs_chain_measure {   /* 40 bytes */
    int32_t axial, diagonal, other;  /* steps between consecutive points, by kind */
    int32_t peak_index;              /* position in `points` of the first point that attains `peak`; -1 if none */
    float   peak, weakest;           /* largest / smallest non-NaN strength; -INFINITY / +INFINITY if none */
    double  sum;                     /* IEEE sum of the chain's strengths (NaN propagates) */
    double  length;                  /* sum of the Euclidean step lengths, in double */
} cvs_chain_measure;
int cvs_chain_measures(cvs_handle h, const int32_t* points, int n_points,
                       const cvs_chain* chains, int n_chains,
                       const float* xy,        /* NULL: lengths from the integer points; else from the sub-pixel pairs */
                       const float* strength,  /* NULL: peak_index -1, peak -INF, weakest +INF, sum 0 */
                       cvs_chain_measure* table, int mem);

/* EXTENSION: contour segments -- table[k] is the total-least-squares line through the points of the polyline span that starts at vertex k
 * of a cvs_chain_polylines result, fitted to the sub-pixel positions of cvs_chain_refine (or to the integer points), weighted by their
 * strengths (or not).  One record per vertex, so the table lines up with `index`: no count, no prefix sum, nothing read back.  Needs no
 * image size (any handle, before or after a setup).
 * SPANS.  Vertex k belongs to polyline c = the largest c with polylines[c].start <= k (the rule of `ranges` in cvs_chain_refine_batch: an
 * entry of length 0 is skipped).  With (S, L, F) = chains[c] and (vs, vl) = polylines[c]: if k + 1 < vs + vl the span is the points at
 * positions index[k] .. index[k+1], both ends included (a vertex belongs to both of its spans); if k is the polyline's last vertex and
 * F has CVS_CHAIN_CLOSED it is the positions index[k] .. S+L-1 followed by S .. index[vs], flag CVS_SEG_WRAPS (a closed chain with one
 * vertex: the whole cycle, L + 1 points); otherwise -- the last vertex of an open polyline -- there is no span.  first = index[k], count =
 * the number of points of the span (>= 2) or 0, chain = c.  A record without a span has first, count = 0, chain, and every other word 0.
 * TERMS.  (x0, y0) = points[first] widened to double.  Per point i of the span dx = (double)xs_i - x0, dy = (double)ys_i - y0 with
 * (xs, ys) from xy when it is given, else the integer point (both differences are exact for |coordinates| < 2^28); the weight wi is 1 when
 * strength == NULL, else (double)strength_i if strength_i > 0 (false for NaN), else 0.  The terms, every operation rounded on its own:
 * wi, wi*dx, wi*dy, (wi*dx)*dx, (wi*dx)*dy, (wi*dy)*dy; w, sx, sy, sxx, sxy, syy are their IEEE double sums in an order fixed by `count`
 * alone (the rule of cvs_chain_measures: a lane adds every 16th term in ascending order where count <= 256, every 256th otherwise, and the
 * lanes are combined by a butterfly): the same call twice gives the same bytes.  No floating-point atomic is used.  The moments are stored so that a caller who merges collinear
 * spans can shift them by the integer offset of the two `first` pixels and add them.
 * LINE.  From the six sums, in double, exactly this sequence (no contraction; division and sqrt correctly rounded):
 *   mx = sx/w; my = sy/w;  a = sxx - sx*mx; b = sxy - sx*my; c = syy - sy*my;  d = a - c; e = b + b; r = sqrt(d*d + e*e);
 *   (vx, vy) = d >= 0 ? (d + r, e) : (e, r - d)   -- the eigenvector of the larger eigenvalue, in the form that does not cancel;
 *   hh = sqrt(vx*vx + vy*vy); ux = vx/hh; uy = vy/hh;
 *   q = the last point's (dx, dy) minus the first point's, s = ux*qx + uy*qy; (ux, uy) is negated if s < 0, or if s == 0 and (ux < 0, or
 *   ux == 0 and uy < 0): the direction runs from the first point towards the last;
 *   cx = x0 + mx; cy = y0 + my;  t0 = ux*(dx_first - mx) + uy*(dy_first - my), t1 the same for the last point: the segment is
 *   (cx, cy) + t * (ux, uy), t in [t0, t1];
 *   lmin = 0.5*((a + c) - r), replaced by 0 unless it is > 0; rms = sqrt(lmin / w): the weighted RMS distance of the points from the line;
 *   dmax = the largest |ux*(dy_i - my) - uy*(dx_i - mx)| over ALL points of the span, whatever their weight (a second pass; a maximum does
 *   not depend on the order).
 * If !(w > 0), !(hh > 0) or hh is infinite -- a NaN anywhere in the span's xy, all weights 0, all points equal -- the flag
 * CVS_SEG_DEGENERATE is set, ux, uy, t0, t1, rms and dmax are NaN, cx and cy are as computed (NaN when w is not > 0), the sums are stored
 * as they came out, and the second pass is skipped.
 * points, chains, polylines, index, xy, strength and table are all in host or all in device memory (mem).  Device arrays: two launches --
 * sixteen lanes per span of up to 256 points, one 256-lane workgroup per longer span -- queued on the handle's stream, nothing read back,
 * capturable; the launch sequence depends on n_vertices alone.  Host arrays are staged in handle scratch (grown only, freed by
 * cvs_destroy), the call synchronises, and it returns CVS_E_UNSUPPORTED while the stream is being captured.  n_vertices == 0: CVS_OK,
 * nothing queued.
 * CVS_E_BADARG, nothing written: a negative count; a required array missing (points with n_points > 0, chains / polylines with
 * n_chains > 0, index / table with n_vertices > 0); n_vertices > 0 with n_chains == 0; an invalid mem; a pointer not aligned to 4 bytes, or
 * to 8 for table; a table that overlaps an input; and, for HOST arrays, a chains entry that violates start >= 0, length >= 1,
 * start + length <= n_points, polylines whose starts are not the running sum of their lengths from 0 to n_vertices, an index that is not
 * strictly increasing inside each polyline or that leaves its chain's [S, S+L).  n_points > 2^30: CVS_E_SIZE.
 * DEVICE tables are trusted for their meaning only: the binary search cannot leave 0 .. n_chains - 1; a vertex whose chain entry fails
 * the three conditions, whose index[k], index[k+1] or index[vs] lies outside [S, S+L), whose index[k] >= index[k+1], or that does not lie
 * inside the polyline the search found, gets the record without a span -- so no load leaves the arrays; coordinates are never used as
 * addresses.  A table of cvs_contour_chains_batch goes through as it is: its starts are global, and `reserved` is not read. */
typedef struct cvs_segment {          /* 128 bytes */
    int32_t first;                    /* index[k]: position in `points` of the span's first point */
    int32_t count;                    /* points of the span, >= 2; 0: no span */
    int32_t chain;                    /* the polyline (= chain) the vertex belongs to */
    int32_t flags;                    /* CVS_SEG_WRAPS = 1, CVS_SEG_DEGENERATE = 2 */
    double  w, sx, sy, sxx, sxy, syy; /* weighted moments about the span's first pixel */
    double  cx, cy;                   /* the weighted centroid: a point of the line */
    double  ux, uy;                   /* unit direction, from the first point towards the last */
    double  t0, t1;                   /* the first and the last point projected on the line: (cx, cy) + t * (ux, uy) */
    double  rms, dmax;                /* weighted RMS and largest distance of the span's points from the line */
} cvs_segment;
enum { CVS_SEG_WRAPS = 1, CVS_SEG_DEGENERATE = 2 };
int cvs_polyline_segments(cvs_handle h,
        const int32_t* points, int n_points,
        const cvs_chain* chains, const cvs_chain* polylines, int n_chains,
        const int32_t* index, int n_vertices,
        const float* xy,        /* NULL: fit the integer points */
        const float* strength,  /* NULL: unit weights */
        cvs_segment* table,     /* n_vertices records */
        int mem);

/* EXTENSION: contour turns -- table[i] says how sharply the contour turns at point i of a point list, and whether the point is a CORNER of
 * its chain: the turn between the direction in which the chain arrives (from the centroid of the `radius` points before it) and the one in
 * which it leaves (towards the centroid of the `radius` points after it).  One fixed-size record per input point, so the table lines up
 * with `points`: no count, no prefix sum, nothing read back.  Needs no image size (any handle, before or after a setup).  No curvature is
 * stored: the record carries the sine, the cosine and the two arm lengths, from which a caller forms what it wants.
 * ARMS.  Point i lies in chain c = (S, L, F) = chains[c] at offset j = i - S.  Open chain: nb = min(radius, j), nf = min(radius, L-1-j); the
 * arm points are the offsets j-k, k = 1 .. nb, and j+k, k = 1 .. nf.  Chain with CVS_CHAIN_CLOSED: nb = nf = min(radius, (L-1)/2) (integer
 * division) and the offsets are taken modulo L, so the two arms never share a point and never contain j itself.
 * SUMS.  All arithmetic is IEEE double, every operation rounded on its own (no contraction).  The coordinates (x, y) of a point are its
 * (xs, ys) pair of `xy` widened to double when xy != NULL, else its integer point.  Term k of the backward arm is
 * (x[j-k] - x[j], y[j-k] - y[j]); sb = term 1 + term 2 + ... + term nb, added in ascending k, x and y separately; sf the same over j+k.
 * ab = sb / (double)nb, af = sf / (double)nf (component by component, correctly rounded): the arm centroids relative to the point.
 * TURN.  din = (-ab.x, -ab.y); cr = din.x*af.y - din.y*af.x; dt = din.x*af.x + din.y*af.y; la = sqrt(ab.x*ab.x + ab.y*ab.y),
 * lf = sqrt(af.x*af.x + af.y*af.y) (sqrt correctly rounded); den = la*lf.  Stored: sin = (float)(cr/den), cos = (float)(dt/den),
 * lb = (float)la, lf = (float)lf; nothing is clamped (|sin|, |cos| may exceed 1 by a rounding).  cos = 1 is a straight chain, 0 a right
 * angle, -1 a reversal.  x grows to the right and y DOWNWARDS, as in every point list here: a positive sine is a CLOCKWISE turn as seen
 * on the screen -- to the right for someone who walks along the chain in its direction -- and a negative one counter-clockwise.
 * FLAGS.  CVS_TURN_END: nb == 0 or nf == 0 (every point of a chain with L == 1, both points of an open chain with L == 2, all points of a
 * closed chain with L <= 2, the two ends of every open chain): sin and cos are NaN, the length of a missing arm is 0 and that of an arm
 * that exists is as computed.  CVS_TURN_DEGENERATE: not END, and !(den > 0) or den is not finite (an arm centroid on the point itself, a
 * NaN or an infinity in xy): sin and cos are NaN, lb and lf as computed.  CVS_TURN_SHORT: nb < min_arm or nf < min_arm (set beside END as
 * well).  Every NaN the call stores is the quiet NaN 0x7FC00000.  A point is ELIGIBLE iff none of END, DEGENERATE, SHORT and NO_CHAIN
 * (below) is set; the cos of an eligible point is finite.
 * CORNER.  CVS_TURN_CORNER is set iff the point is eligible, its stored cos <= max_cos (float comparison), and for every k = 1 .. nms
 * (closed chains: k <= (L-1)/2 as well) whose neighbour at offset j-k / j+k exists and is eligible: cos_i < cos_(j-k) (strict backwards)
 * and cos_i <= cos_(j+k).  Open chains skip offsets outside [0, L); closed chains wrap modulo L.  This is the plateau rule of cvs_nonmax
 * applied to the smaller cosine: of equal cosines side by side the first wins (on a closed chain whose equal minima follow each other
 * within nms all the way round none is the first, and none is a corner).  A point that is not eligible is never a corner and never
 * suppresses one.  nms == 0: every eligible point with cos <= max_cos is a corner.
 * SUMMARY (may be NULL).  summary[c]: corners / eligible = the number of points of chain c with CVS_TURN_CORNER / that are eligible;
 * sharpest = the position in `points` of the eligible point with the smallest cos, the first on ties, -1 if there is none; min_cos = that
 * cos, +INFINITY if there is none.  Only records whose `chain` is c count.  Integers and a minimum with a first-index tie rule: the order
 * of evaluation does not matter.
 * TABLES.  The chain of point i is the largest c with chains[c].start <= i (the rule of cvs_polyline_segments).  HOST tables are checked
 * in full: CVS_E_BADARG unless the starts are the running sum of the lengths from 0 to n_points and every length is >= 1 (so n_points > 0
 * needs n_chains > 0).  DEVICE tables are trusted for their meaning only: the search is a binary search that cannot leave
 * 0 .. n_chains - 1 and finds that c whenever the starts ascend (which entry it finds where they do not is unspecified); a point that does
 * not lie inside the entry found -- S < 0, L < 1, S + L > n_points, i < S or i >= S + L -- gets chain -1, flags CVS_TURN_NO_CHAIN, nb =
 * nf = 0, lb = lf = 0 and NaN in sin and cos, and an entry that fails the first three conditions gets the summary of a chain without
 * points (0, 0, -1, +INFINITY).  So no load leaves the arrays; coordinates are never used as addresses.  A table of
 * cvs_contour_chains_batch goes through as it is: its starts are global, and `reserved` is not read.
 * points, chains, xy, table and summary are all in host or all in device memory (mem).  Device arrays: two launches, three with summary
 * -- one lane per point for the turns, one lane per point for the corners, one wave per chain of up to 256 points and one 256-lane
 * workgroup per longer chain for the summary -- queued on the handle's stream, nothing read back, capturable; the launch sequence depends
 * on (n_points, n_chains, summary != NULL) alone.  The result is a function of the inputs alone: the same call twice gives the same
 * bytes.  No floating-point atomic is used.  Host arrays are staged in handle scratch (grown only, freed by cvs_destroy), the call
 * synchronises, and it returns CVS_E_UNSUPPORTED while the stream is being captured.  n_points == 0: CVS_OK, nothing queued and nothing
 * written (summary included).
 * CVS_E_BADARG, nothing written: cfg NULL, radius outside 1 .. 64, min_arm outside 1 .. radius, nms outside 0 .. 64, max_cos NaN or outside
 * -1 .. 1; a negative count; a required array missing (points / table with n_points > 0, chains with n_chains > 0); n_points > 0 with
 * n_chains == 0; an invalid mem; a pointer not aligned to 4 bytes; table or summary overlapping an input or each other; a HOST table as
 * above.  n_points > 2^30: CVS_E_SIZE. */
typedef struct cvs_turn_cfg {
    int32_t radius;    /* 1..64: points per arm */
    int32_t min_arm;   /* 1..radius: a point with a shorter arm is never a corner and never suppresses one */
    int32_t nms;       /* 0..64: half window of the 1-D non-maximum suppression; 0 = none */
    float   max_cos;   /* a corner has cos <= max_cos; -1..1, NaN refused */
} cvs_turn_cfg;
typedef struct cvs_chain_turn {      /* 32 bytes */
    int32_t chain;                   /* the chain the point belongs to; -1: none (device tables only) */
    int32_t flags;                   /* CVS_TURN_CORNER = 1, CVS_TURN_END = 2, CVS_TURN_DEGENERATE = 4, CVS_TURN_SHORT = 8, CVS_TURN_NO_CHAIN = 16 */
    int32_t nb, nf;                  /* points in the backward / forward arm */
    float   sin, cos;                /* of the turn from the incoming to the outgoing direction; sin > 0: clockwise on the screen */
    float   lb, lf;                  /* distance of the arm centroids from the point */
} cvs_chain_turn;
enum { CVS_TURN_CORNER = 1, CVS_TURN_END = 2, CVS_TURN_DEGENERATE = 4, CVS_TURN_SHORT = 8, CVS_TURN_NO_CHAIN = 16 };
typedef struct cvs_turn_summary {    /* 16 bytes, one per chain */
    int32_t corners, eligible;       /* points of the chain with CVS_TURN_CORNER / that are eligible */
    int32_t sharpest;                /* position in `points` of the eligible point with the smallest cos, the first on ties; -1 */
    float   min_cos;                 /* +INFINITY if none */
} cvs_turn_summary;
int cvs_chain_turns(cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, int n_chains,
                    const float* xy,            /* NULL: the integer points */
                    const cvs_turn_cfg* cfg,
                    cvs_chain_turn* table,      /* n_points records */
                    cvs_turn_summary* summary,  /* NULL, or n_chains records */
                    int mem);

/* EXTENSION: contour joins -- what cvs_contour_chains took away when it cut the contours at their junctions: table[2c] and table[2c+1]
 * say which other chain ends lie at the same node as the head and the tail of chain c, and which of them continues the chain most nearly
 * straight.  One fixed-size record per chain END, so the table lines up with `chains`: no count, no prefix sum, nothing read back.  Needs
 * no image size (any handle, before or after a setup).  Stitching chains into paths over the MUTUAL joins is cvs_chain_paths, below.
 * ENDS.  Chain c = (S, L, F, R) = chains[c].  Its head, end 2c, sits at position j = S and its arm runs forwards (sign +1); its tail, end
 * 2c+1, sits at j = S+L-1 and its arm runs backwards (sign -1).  A chain with CVS_CHAIN_CLOSED or with L < 2 has no ends: both its
 * records are node = next = partner = -1, degree = n = 0, cos = sin = NaN, flags = CVS_JOIN_NONE.  Every NaN the call stores is the quiet
 * NaN 0x7FC00000.
 * NODE.  The key of an end is (R, y, x) of its INTEGER point, whether xy is given or not.  R is the fourth word of the entry -- 0 from
 * cvs_contour_chains, the plane from cvs_contour_chains_batch -- and it IS READ here, unlike in cvs_polyline_segments and cvs_chain_turns:
 * ends of different planes never share a node, so a batch table goes through as it is.  Ends with equal keys are at the same node.  node =
 * the smallest end number at the node, degree = the number of ends there (this one included), next = the next larger end number there,
 * wrapping from the largest to the smallest (its own number when degree is 1): following next visits the node's ends in a ring.  A loop
 * that leaves and re-enters a junction has both its ends at one node; they may be partners.  degree > 8: CVS_JOIN_CROWDED on every end of
 * the node -- node and degree are right, n and the arm's own flags are as computed, next = partner = -1, cos = sin = NaN.  (Never on a
 * table of cvs_contour_chains: a pixel has at most 4 links, so degree <= 4 there, and never exactly 2.)
 * ARM.  The arm of cvs_chain_turns at a chain end: n = min(radius, L-1) points; term k = (x[j +- k] - x[j], y[j +- k] - y[j]), k = 1 .. n,
 * where the coordinates of a point are its (xs, ys) pair of `xy` widened to double when xy != NULL, else its integer point.  All
 * arithmetic is IEEE double, every operation rounded on its own (no contraction): the terms are added in ascending k, starting from term
 * 1, x and y separately; a = sum / (double)n (component by component, correctly rounded); len = sqrt(a.x*a.x + a.y*a.y) (correctly
 * rounded).  CVS_JOIN_SHORT iff n < min_arm.  CVS_JOIN_DEGENERATE iff !(len > 0) or len is not finite (an arm centroid on the end itself,
 * a NaN or an infinity in xy).  An end is ELIGIBLE iff none of NONE, CROWDED, SHORT, DEGENERATE and NO_CHAIN (below) is set.
 * PAIR.  For eligible ends e != f at one node, with lo = min(e, f), hi = max(e, f): den = len_lo*len_hi; dt = -(a_lo.x*a_hi.x +
 * a_lo.y*a_hi.y); cr = a_lo.y*a_hi.x - a_lo.x*a_hi.y.  cos(e,f) = (float)(dt/den) in both directions; sin(lo,hi) = (float)(cr/den) and
 * sin(hi,lo) = sin(lo,hi) with its sign bit flipped.  Nothing is clamped (|cos| may exceed 1 by a rounding); from float coordinates den
 * neither overflows nor underflows, so the cos and sin of an eligible pair are finite.  They are the turn of cvs_chain_turns with the
 * arriving direction -a_e and the leaving direction a_f: cos = 1 is a straight continuation, sin > 0 a CLOCKWISE turn on the screen (y
 * grows downwards).  So cos(e,f) and cos(f,e) are the same bits and sin(e,f), sin(f,e) differ in the sign bit alone, zeros included --
 * the pair is evaluated once, from its smaller end, because cr taken from the larger end would be +0 again wherever the two products
 * are equal (every straight diagonal continuation).
 * PARTNER.  partner(e) = the eligible f != e at e's node with the largest cos(e,f), a float comparison: candidates are visited in
 * ascending f and replace the one held only on strictly greater, so the smallest f wins a tie and +0 ties with -0.  cos and sin are
 * those of (e, partner).  No candidate: partner = -1, cos = sin = NaN.  An end that is not eligible has partner -1 and NaN, and is
 * nobody's partner.  CVS_JOIN_MUTUAL iff partner(partner(e)) == e and cos >= min_cos (float comparison).  MUTUAL joins pair ends off:
 * partner is an involution on the ends that carry the flag, so following MUTUAL joins from any end never branches.
 * TABLES.  As in cvs_chain_turns: HOST tables are checked in full -- CVS_E_BADARG unless the starts are the running sum of the lengths
 * from 0 to n_points and every length is >= 1.  DEVICE tables are trusted for their meaning only: an entry that fails S >= 0, L >= 1,
 * S + L <= n_points gets the records of a chain without ends with CVS_JOIN_NO_CHAIN added (flags = NONE | NO_CHAIN) and enters no node;
 * nothing else is asked of the table (entries may overlap or leave gaps).  So no load and no store leaves the arrays; coordinates are
 * never used as addresses.
 * points, chains, xy and table are all in host or all in device memory (mem).  Device arrays: three launches, one lane per end in each
 * -- the arms, the grouping of the ends by key in a hash table, the records -- queued on the handle's stream, nothing read back, nothing
 * synchronised, capturable; the launch sequence depends on n_chains alone.  The result is a function of the inputs alone: the same call
 * twice gives the same bytes (which slot of the hash table a node gets depends on a race; no output does).  Integer atomics only; no
 * floating-point atomic is used.  The grouping needs handle scratch (grown only, freed by cvs_destroy): 112 bytes per chain and 16 bytes
 * per slot of a table of max(8, the power of two >= 4 n_chains) slots -- at most 240 bytes per chain.  A call that would have to GROW the
 * scratch while the stream is being captured returns CVS_E_UNSUPPORTED ("call once eagerly first", the rule of cvs_link); the handle works
 * on.  Host arrays are staged in the same scratch, the call synchronises, and it returns CVS_E_UNSUPPORTED while the stream is being
 * captured.  n_chains == 0: CVS_OK, nothing queued and nothing written.
 * CVS_E_BADARG, nothing written: cfg NULL, radius outside 1 .. 64, min_arm outside 1 .. radius, min_cos NaN or outside -1 .. 1, reserved
 * != 0; a negative count; a required array missing (points with n_points > 0, chains / table with n_chains > 0); n_points > 0 with
 * n_chains == 0; an invalid mem; a pointer not aligned to 4 bytes; table overlapping an input; a HOST table as above.  n_points > 2^30 or
 * n_chains > 2^26: CVS_E_SIZE. */
typedef struct cvs_join_cfg {
    int32_t radius;    /* 1..64: points per arm */
    int32_t min_arm;   /* 1..radius: an end with a shorter arm joins nothing and is nobody's partner */
    float   min_cos;   /* -1..1, NaN refused: CVS_JOIN_MUTUAL needs cos >= min_cos */
    int32_t reserved;  /* 0 */
} cvs_join_cfg;
typedef struct cvs_chain_join {      /* 32 bytes, one per chain END: record 2c = head of chain c, 2c+1 = tail */
    int32_t node;                    /* the smallest end number at the same node; -1: the end does not exist */
    int32_t degree;                  /* ends at the node, this one included */
    int32_t next;                    /* the next larger end at the node, cyclically (== own number when degree 1); -1 */
    int32_t partner;                 /* the end that continues this one most nearly straight; -1 */
    int32_t flags;                   /* CVS_JOIN_MUTUAL = 1, _NONE = 2, _CROWDED = 4, _SHORT = 8, _DEGENERATE = 16, _NO_CHAIN = 32 */
    int32_t n;                       /* points of the arm */
    float   cos, sin;                /* of the turn from arriving through this end to leaving through `partner`; NaN without partner */
} cvs_chain_join;
enum { CVS_JOIN_MUTUAL = 1, CVS_JOIN_NONE = 2, CVS_JOIN_CROWDED = 4, CVS_JOIN_SHORT = 8, CVS_JOIN_DEGENERATE = 16, CVS_JOIN_NO_CHAIN = 32 };
int cvs_chain_joins(cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, int n_chains,
                    const float* xy,            /* NULL: the integer points */
                    const cvs_join_cfg* cfg,
                    cvs_chain_join* table,      /* 2 * n_chains records */
                    int mem);

/* EXTENSION: contour paths -- the chains of a chain table put back together over the MUTUAL joins of cvs_chain_joins: (points, chains,
 * joins) becomes (path_points, paths), and `paths` is again a chain table that obeys the running-sum rule, so every chain-array call
 * (cvs_chain_polylines, cvs_chain_measures, cvs_polyline_segments, cvs_chain_turns, cvs_chain_joins itself) runs on whole contours as
 * it is.  All outputs are sized by the inputs: no sizing call, no capacity, nothing read back.  Integer arithmetic only; coordinates are
 * copied, never compared.  Needs no image size.
 * ENTRIES, ENDS, LINKS.  Entry c = (S, L, F, R) = chains[c] is VALID iff S >= 0, L >= 1 and S + L <= n_points.  A valid entry HAS ENDS
 * iff L >= 2 and CVS_CHAIN_CLOSED is not set: end 2c is its head (position S), end 2c+1 its tail (position S+L-1).  End e is LINKED iff,
 * with p = joins[e].partner: chain e>>1 has ends, joins[e].flags has CVS_JOIN_MUTUAL, 0 <= p < 2 n_chains, p != e, chain p>>1 has ends,
 * joins[p].flags has CVS_JOIN_MUTUAL and joins[p].partner == e.  The test is symmetric, so the linked ends are paired off whatever bytes
 * the join table holds; p == e^1 is allowed (a loop whose two ends continue each other).  No other field of a join record is read.
 * WALKS.  Entering a chain through end e lists its positions from e's position to the other end's: even e gives S .. S+L-1, odd e gives
 * S+L-1 .. S.  succ(e) = joins[e^1].partner if LINKED(e^1), else none: out through the other end, into its partner.  Every end has at
 * most one successor and one predecessor, so the entry ends form disjoint lists and cycles.  Every path appears as two TWIN walks, each
 * the other reversed with every e replaced by e^1; twins are never the same walk.
 * CANONICAL WALK.  Open path: the twin whose first entry end is the smaller number.  Cycle: the twin that contains the smallest end
 * number of the two, started at that end (always a head, so that chain goes forward).  A valid entry without ends is a path of one
 * member, entry end 2c, not reversed.  An invalid entry (DEVICE memory only) makes no path, no member and no point.  Paths are sorted
 * ascending by their first entry end; the members of a path are in walk order.
 * POINTS.  Member k >= 1 drops its first position (the junction pixel the member before it listed); a cycle also drops the last
 * position of its last member; the rest go, in order, into path_points, and where given into index (the position in `points`) and
 * path_xy (the bits of xy).  A member may emit no point at all (a cycle's last member with L = 2).
 * RECORDS.  paths[p] = (start, length, flags, R of the first member's chain): the starts are the running sum of the lengths; flags is
 * CVS_CHAIN_CLOSED for a cycle or a closed member, else CVS_CHAIN_HEAD_JUNCTION from the junction bit of the first entry end (entering
 * through a head reads the chain's HEAD_JUNCTION, through a tail its TAIL_JUNCTION) and CVS_CHAIN_TAIL_JUNCTION likewise from the last
 * member's exit end.  info[p] = (first member, number of members, first entry end, exit end of the last member).  members[m] = (chain,
 * CVS_MEMBER_REVERSED iff entered through the tail, path, index in path_points of its first emitted point -- where that point would be
 * if it emits none).  counts = (n_paths, n_path_points); records and points past the counts are not written.
 * IT FOLLOWS that n_path_points = (points of valid entries) - (linked pairs), n_paths = (valid entries) - (linked pairs) + (cycles),
 * members = valid entries; and that with no linked end and a table that obeys the running-sum rule the outputs are the inputs: paths
 * == chains byte for byte (for flags the library writes), path_points == points, index = 0 .. n-1, members[c] = (c, 0, c, S).
 * MEMORY.  All arrays are in host or all in device memory (mem).  HOST: `chains` is checked in full -- CVS_E_BADARG unless the starts are
 * the running sum of the lengths from 0 to n_points and every length is >= 1 (the join table needs no check: LINKED is total); the
 * arrays are staged in handle scratch, the call synchronises, and it returns CVS_E_UNSUPPORTED while the stream is being captured.
 * DEVICE: tables are trusted for nothing -- every index is checked before it is an address, no load and no store leaves the arrays;
 * entries may overlap or leave gaps, and where overlapping valid entries add up to more than n_points points the sums (starts, lengths,
 * counts) are formed modulo 2^32 and points at an index >= n_points are not stored.
 * EXECUTION.  One lane per end: links, pointer jumping over the walks between two buffers (first along succ for each walk's last and
 * smallest end, then, with every cycle cut in front of its smallest end, along pred for each member's rank and point offset), a scan
 * over the ends that numbers the paths and sums their lengths and members, the records, the points.  2 * ceil(log2(n_chains)) + 8
 * launches (8 for n_chains == 1), a function of n_chains alone -- a table of arbitrary bytes takes the same launches as a good one; no
 * kernel has a loop without a static bound, none waits or spins, none uses an atomic.  Queued on the handle's stream, nothing read
 * back, nothing synchronised, capturable.  The same call twice gives the same bytes.  Handle scratch (grown only, freed by cvs_destroy):
 * CVS_PATH_SCRATCH_PER_END = 80 bytes per end, 160 per chain, and 12 bytes per 1024 ends.  A call that would have to GROW the scratch
 * while the stream is being captured returns CVS_E_UNSUPPORTED ("call once eagerly first", the rule of cvs_chain_joins); the handle
 * works on.  n_chains == 0: counts = (0, 0), CVS_OK.
 * CVS_E_BADARG, nothing written: a negative count; a required array missing (counts; points / path_points with n_points > 0; chains /
 * joins / paths / info / members with n_chains > 0); path_xy without xy or xy without path_xy; n_points > 0 with n_chains == 0; an
 * invalid mem; a pointer not aligned to 4 bytes; an output overlapping an input or another output; a HOST table as above.  n_points >
 * 2^30 or n_chains > 2^26: CVS_E_SIZE. */
typedef struct cvs_path_member {     /* 16 bytes, one per valid chain, in path and walk order */
    int32_t chain;
    int32_t flags;                   /* CVS_MEMBER_REVERSED = 1: entered through its tail, its points run backwards */
    int32_t path;
    int32_t start;                   /* index in path_points of its first emitted point */
} cvs_path_member;
typedef struct cvs_path_info {       /* 16 bytes, one per path */
    int32_t first_member, n_members; /* members[first_member .. first_member + n_members) */
    int32_t first_end, last_end;     /* the first member's entry end, the last member's exit end */
} cvs_path_info;
enum { CVS_MEMBER_REVERSED = 1 };
enum { CVS_PATH_SCRATCH_PER_END = 80 };
int cvs_chain_paths(cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, int n_chains,
                    const cvs_chain_join* joins,      /* 2 * n_chains records, as cvs_chain_joins writes them */
                    const float* xy,                  /* NULL, or n_points (xs, ys) pairs */
                    int32_t* path_points,             /* room for n_points (x, y) pairs */
                    cvs_chain* paths,                 /* room for n_chains entries */
                    cvs_path_info* info,              /* room for n_chains records */
                    cvs_path_member* members,         /* room for n_chains records */
                    int32_t* index,                   /* NULL, or room for n_points: path point k is points[index[k]] */
                    float* path_xy,                   /* required iff xy != NULL: room for n_points pairs */
                    int32_t* counts,                  /* 2 ints, same mem: n_paths, n_path_points */
                    int mem);

/* EXTENSION: contour bridges -- the gaps hysteresis leaves in a contour, closed: two FREE chain ends that face each other across a few
 * missing pixels are paired off, and each pair is given a BRIDGE, a digital line from the one end pixel to the other.  A bridge is an
 * ordinary chain appended to the chain table: (points, chains) becomes (out_points, out_chains), and on that pair cvs_chain_joins finds
 * a node of degree 2 at either end pixel of a bridge and cvs_chain_paths stitches through it, listing the shared pixel once.  One
 * fixed-size record per chain END says what became of the end.  Needs no image size.
 * ENDS AND ARMS are those of cvs_chain_joins, to the bit.  Chain c = (S, L, F, R) = chains[c]; its head, end 2c, sits at position j = S
 * (sign +1), its tail, end 2c+1, at j = S+L-1 (sign -1).  A chain with CVS_CHAIN_CLOSED or L < 2 has no ends: both its records are
 * partner = bridge = start = -1, n = steps = 0, cos = cos_partner = NaN (every NaN stored is 0x7FC00000), flags = CVS_BRIDGE_NONE.  The
 * arm: n = min(radius, L-1) points; term k = (x[j +- k] - x[j], y[j +- k] - y[j]), the coordinates of a point being its pair of `xy`
 * widened to double when xy != NULL, else its integer point; IEEE double, every operation rounded on its own, the terms added in
 * ascending k starting from term 1; a = sum / (double)n, len = sqrt(a.x*a.x + a.y*a.y), both correctly rounded.  CVS_BRIDGE_SHORT iff
 * n < min_arm; CVS_BRIDGE_DEGENERATE iff !(len > 0) or len is not finite.
 * FREE.  An end is FREE iff its junction bit in F is clear -- the head reads CVS_CHAIN_HEAD_JUNCTION, the tail CVS_CHAIN_TAIL_JUNCTION; an
 * end that exists and is not free gets CVS_BRIDGE_JUNCTION.  Only those two bits and CVS_CHAIN_CLOSED are read of F, so a table of
 * cvs_contour_chains / _batch and a table of cvs_chain_paths (whose flags carry the junction bits of a path's outer ends) both go
 * through as they are.  A CANDIDATE is an end with none of NONE, NO_CHAIN, JUNCTION, SHORT, DEGENERATE and CROWDED (below).
 * CROWDING, the static bound.  The cell of an end is (R, floor(y / max_gap), floor(x / max_gap)) of its INTEGER point (floor division:
 * coordinates may be negative).  The ends that would be candidates but for CROWDED are counted per cell; a cell that holds more than
 * CVS_BRIDGE_MAX_CELL = 32 of them is crowded, and every end that exists and has a crowded cell among the 3 x 3 cells around its own
 * (same R) gets CVS_BRIDGE_CROWDED: it has no partner and is nobody's candidate.  Every end within max_gap of an end lies in those nine
 * cells, so no end is ever compared with more than 9 x 32 others.
 * PAIR.  For candidates e != f with the same plane word R, lo = min(e, f), hi = max(e, f); f == e^1 is allowed (a contour that nearly
 * closes on itself).  On the INTEGER points, in 64-bit integers: dx = x_hi - x_lo, dy = y_hi - y_lo, steps = max(|dx|, |dy|), d2 =
 * dx*dx + dy*dy.  The pair is IN RANGE iff 2 <= steps <= max_gap.  In doubles, with D = coords(hi) - coords(lo) (coords as for the
 * arm) and dlen = sqrt(D.x*D.x + D.y*D.y): cos_lo = (float)(-(a_lo.x*D.x + a_lo.y*D.y) / (len_lo*dlen)), cos_hi = (float)((a_hi.x*D.x +
 * a_hi.y*D.y) / (len_hi*dlen)) -- 1 where the end points straight at the other.  The pair is always evaluated from lo, so both ends see
 * the same bits.  It is ADMISSIBLE iff it is in range, dlen is finite and > 0, and cos_lo >= min_cos and cos_hi >= min_cos (float
 * comparisons: false for NaN).
 * PARTNER.  partner(e) = the f of the admissible pairs (e, f) with the smallest (d2, f), lexicographically; steps, cos (this end's
 * cosine) and cos_partner (the partner's) are those of that pair.  None: partner = -1, steps = 0, NaN.  CVS_BRIDGE_MUTUAL iff
 * partner(partner(e)) == e: admissibility and d2 are symmetric, so MUTUAL pairs ends off.
 * BRIDGES.  The MUTUAL pairs are numbered by ascending lo.  Bridge k has steps+1 points and is chain n_chains + k; its first point is
 * out_points[n_points + (sum of steps+1 over the bridges before it)].  Point j = 0 .. steps is (x_lo + floor((2*j*dx + steps) /
 * (2*steps)), y_lo + floor((2*j*dy + steps) / (2*steps))) in 64-bit integers: an 8-connected line whose point 0 is lo's pixel and whose
 * point `steps` is hi's.  Its entry is (start, steps+1, CVS_CHAIN_HEAD_JUNCTION | CVS_CHAIN_TAIL_JUNCTION, R).  With xy, out_xy of its
 * points 0 and steps are the bits of the two ends' xy and of point j between them (float)(c_lo + t*(c_hi - c_lo)), t = (double)j /
 * (double)steps, per coordinate, every operation rounded in double.  out_points[0 .. n_points), out_xy[0 .. n_points) and out_chains[0 ..
 * n_chains) are copies of the inputs, with the junction bit of every MUTUAL end set in the copy of its chain's flags (so the next
 * cvs_chain_bridges leaves it alone and a path through it reads as continued).  table[e].bridge and .start are k and the index of the
 * bridge's first point, on both ends of the pair; -1 on every other end.
 * CAPACITIES.  counts = (n_bridges, n_chains + n_bridges, n_points + all bridge points): the full totals, always.  Bridge k is WRITTEN
 * iff n_chains + k < cap_chains and the index of its last point is < cap_points -- a prefix of the bridges; no entry and no point of
 * another bridge is touched, and nothing past the capacities ever.  The table does not depend on the capacities.  With out_points ==
 * NULL (then out_chains and out_xy are NULL and both capacities 0) only the table and the counts are written: the sizing call.
 * n_points + bridge points stays below 2^32; where it passes 2^31 - 1, counts[2] and start hold its low 32 bits (no such bridge is ever
 * written: cap_points is an int).
 * MEMORY.  All arrays are in host or all in device memory (mem).  HOST: `chains` is checked in full -- CVS_E_BADARG unless the starts are
 * the running sum of the lengths from 0 to n_points and every length is >= 1; the arrays are staged in handle scratch, the call
 * synchronises, copies out the table, the counts and what was written of the outputs, and returns CVS_E_UNSUPPORTED while the stream is
 * being captured.  DEVICE: tables are trusted for nothing -- an entry that fails S >= 0, L >= 1, S + L <= n_points gets the records of a
 * chain without ends with CVS_BRIDGE_NO_CHAIN added (its copy in out_chains is still the entry as it is); entries may overlap or leave
 * gaps; every index is checked before it is an address and coordinates are never addresses, so no load and no store leaves the arrays.
 * EXECUTION.  One lane per end: the arms and cells, the grouping of the candidates by cell in a hash table, the crowding, the choice
 * of the partner, MUTUAL; a scan over the ends that numbers the bridges and sums their points; the records and entries; then one lane
 * per output point, each bridge point computed on its own.  8 launches, 9 with outputs, whatever the arrays hold -- arrays of
 * arbitrary bytes take the same launches as good ones; no kernel has a loop without a static bound, none waits or spins, the atomics
 * are integer.  Queued on the handle's stream, nothing read back, nothing synchronised, capturable.  The result is a function of the
 * inputs alone: the same call twice gives the same bytes (which slot a cell gets and the order of its list depend on a race; no output
 * does).  Handle scratch (grown only, freed by cvs_destroy): CVS_BRIDGE_SCRATCH_PER_CHAIN = 244 bytes per chain (120 per end, 4 per
 * possible bridge), 16 bytes per slot of a table of max(8, the power of two >= 4 n_chains) slots, 8 bytes per 1024 ends and less than
 * 2 KiB of rounding.  A call that would have to GROW the scratch while the stream is being captured returns CVS_E_UNSUPPORTED ("call
 * once eagerly first", the rule of cvs_chain_joins); the handle works on.  n_chains == 0: counts = (0, 0, 0), CVS_OK.
 * CVS_E_BADARG, nothing written: cfg NULL, radius outside 1 .. 64, min_arm outside 1 .. radius, max_gap outside 2 .. 32, min_cos NaN or
 * outside -1 .. 1; a negative count; a required array missing (counts; points with n_points > 0; chains / table with n_chains > 0);
 * out_points without out_chains or the reverse; a capacity != 0 without its array; cap_points < n_points or cap_chains < n_chains;
 * out_xy without xy or without out_points, or xy and out_points without out_xy; n_points > 0 with n_chains == 0; an invalid mem; a
 * pointer not aligned to 4 bytes; an output overlapping an input or another output; a HOST table as above.  n_points > 2^30 or n_chains
 * > 2^26: CVS_E_SIZE.
 * Out of scope: bridging a free end to the SIDE of a contour, testing the line against the mask, a strength for bridge points. */
typedef struct cvs_bridge_cfg {
    int32_t radius;    /* 1..64: points per arm, the arm of cvs_chain_joins */
    int32_t min_arm;   /* 1..radius: an end with a shorter arm bridges nothing */
    int32_t max_gap;   /* 2..32: largest Chebyshev distance between the two end pixels */
    float   min_cos;   /* -1..1, NaN refused: each end must point at the other within this cone */
} cvs_bridge_cfg;
typedef struct cvs_chain_bridge {    /* 32 bytes, one per chain END: record 2c = head of chain c, 2c+1 = tail */
    int32_t partner;                 /* the free end this one would bridge to; -1 */
    int32_t flags;                   /* CVS_BRIDGE_MUTUAL = 1, _NONE = 2, _JUNCTION = 4, _SHORT = 8, _DEGENERATE = 16, _NO_CHAIN = 32, _CROWDED = 64 */
    int32_t n;                       /* points of the arm */
    int32_t steps;                   /* Chebyshev distance to partner; 0 without */
    int32_t bridge;                  /* number of the bridge, on both ends of a MUTUAL pair; -1 */
    int32_t start;                   /* index in out_points of the bridge's first point; -1 */
    float   cos, cos_partner;        /* this end's and the partner's pointing cosine; NaN without partner */
} cvs_chain_bridge;
enum { CVS_BRIDGE_MUTUAL = 1, CVS_BRIDGE_NONE = 2, CVS_BRIDGE_JUNCTION = 4, CVS_BRIDGE_SHORT = 8, CVS_BRIDGE_DEGENERATE = 16,
       CVS_BRIDGE_NO_CHAIN = 32, CVS_BRIDGE_CROWDED = 64 };
enum { CVS_BRIDGE_SCRATCH_PER_CHAIN = 244, CVS_BRIDGE_MAX_GAP = 32, CVS_BRIDGE_MAX_CELL = 32 };
int cvs_chain_bridges(cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, int n_chains,
                      const float* xy,                         /* NULL: the integer points */
                      const cvs_bridge_cfg* cfg,
                      cvs_chain_bridge* table,                 /* 2 * n_chains records */
                      int32_t* out_points, int cap_points,     /* NULL/0, or room for cap_points >= n_points pairs */
                      cvs_chain* out_chains, int cap_chains,   /* NULL/0, or room for cap_chains >= n_chains entries */
                      float* out_xy,                           /* required iff xy != NULL and out_points != NULL */
                      int32_t* counts,                         /* 3 ints, same mem: n_bridges, n_out_chains, n_out_points */
                      int mem);

/* ---- EXTENSION beyond the reference: the contour chain on the batch axis -- cvs_link, cvs_nonmax_batch, cvs_contours_batch ----
 * None of the three reads anything back: with device planes they queue a launch sequence that depends on the image size, the number of
 * planes and how the planes lie in memory (one constant stride, or not) -- never on what the planes hold -- and return. */

/* EXTENSION: hysteresis and prune in ONE labelling.  in: n >= 1 f32 planes of the handle's image size (typically the thinned maps of
 * many frames; no upper limit on n).  Per plane, W = { pixels with v > low } (NaN is never in W); a component of W (8-connected) is
 * KEPT iff its largest value is > high, its area is >= min_area, and its largest value is >= min_peak (IEEE float comparisons;
 * min_peak = -INFINITY switches the last test off).  out: 255 on the pixels of kept components, 0 elsewhere; all CVS_DEPTH_U8 or all f32
 * (255.0f / 0.0f), as in cvs_hysteresis.  kept_dev: NULL, or n ints in DEVICE memory that receive the number of components kept per
 * plane; no count comes back to the host.
 * Equivalence: byte for byte, and count for count, cvs_link(in, low, high, min_area, min_peak) is cvs_hysteresis(in, low, high)
 * followed by cvs_contour_prune(mask = that, weight = in, min_area, min_peak): the mask hysteresis keeps is exactly the set of
 * W-components that hold a strong pixel, and distinct W-components are never 8-adjacent, so relabelling that mask finds the same
 * components with the same area and peak.  The output is a function of the inputs alone.
 * Fixed, asynchronous, capturable: four launches per chain of planes (tiles, borders, statistics at the roots, emit), all planes of a
 * chain in each; a chain holds as many planes as fit 1 GiB with their parent, area and peak planes (12 bytes per pixel; at least one), so the launch
 * sequence depends on (rows, cols, n) and on whether the planes lie at one constant stride (an [N, H, W] block: addressed
 * arithmetically) or not (a device table that launches fill from their arguments, 16 planes each).  No stream synchronisation and no
 * copy to the host when all planes are device planes.  Under stream capture the call works provided the handle's scratch already has
 * the size it needs (the same call, made once eagerly, sees to that); otherwise CVS_E_UNSUPPORTED, and the handle works on.  Host
 * planes are staged on the device, at most eight planes per chain, synchronise, and are refused during capture.
 * low > high, a NaN threshold, min_area < 0, NaN min_peak, n < 1, outputs of mixed depth, any overlap of an output with an input or
 * another output: CVS_E_BADARG; a plane of another size than the handle's image, or rows * cols > 2^31 - 2 (the limit of cvs_label, and
 * the only one: any height goes): CVS_E_SIZE; no image size yet: CVS_E_STATE.  Nothing is written when an argument is rejected. */
int cvs_link(cvs_handle h, int n, const cvs_plane* in, float low, float high, int min_area, float min_peak,
             const cvs_plane* out, int32_t* kept_dev);

/* EXTENSION: cvs_nonmax for `frames` frames of n_maps (1..3) maps each.  in / out: flat, frame-major arrays of frames * n_maps f32
 * planes; theta: `frames` planes, or NULL = the CVS_PLANE_THETA state plane of frames 0 .. frames - 1 of the last cvs_pipeline_batch
 * (CVS_E_STATE if the handle holds fewer frames, or no orientation state).  Every value is bit for bit that of cvs_nonmax on the same
 * frame (the same kernel body).  ONE launch when the planes are on the device and the theta planes, and map k's in and out planes,
 * each lie at a constant frame stride (an [F][K][H][W] block, the state blocks of a batch); otherwise one cvs_nonmax per frame.
 * Errors as in cvs_nonmax; asynchronous on the handle's stream and capturable (device planes). */
int cvs_nonmax_batch(cvs_handle h, int frames, int n_maps, const cvs_plane* theta, const cvs_plane* in, const cvs_plane* out);

/* EXTENSION: thin, linked contours of n frames: cvs_pipeline_batch (state kept) -> the three maps of every frame in the handle's
 * own scratch -> cvs_nonmax_batch(theta = NULL) -> cvs_link over the wanted planes.  outs: n * 3 planes, frame-major, {edges, dark,
 * bright} per frame, all CVS_DEPTH_U8 or all f32; an entry with data == NULL is not wanted.  Every mask equals, byte for byte, what
 * cvs_pipeline -> cvs_nonmax(theta = NULL) -> cvs_link(low, high, min_area, min_peak) writes for that frame alone on a handle of the
 * same kind and options (G2, or G4 with CVS_OPT_G4_EXTENSIONS).  Afterwards the handle holds the state of all n frames, as after
 * cvs_pipeline_batch.  CVS_OPT_PERSIST_STATE = 0: CVS_E_STATE (thinning needs the theta plane of every frame).  With device planes
 * the call returns without synchronising; n = 1 is valid.  Threshold errors as in cvs_link; an output that overlaps the image of ANY
 * frame, or another output: CVS_E_BADARG; frame errors as in cvs_pipeline_batch. */
int cvs_contours_batch(cvs_handle h, const cvs_plane* images, int n, float low, float high, int min_area, float min_peak,
                       const cvs_plane* outs);

/* ---- EXTENSION beyond the reference: contour chains and sub-pixel chain points on the batch axis ----
 * cvs_contour_chains_batch lists the chains of n masks -- the [n][3] masks of cvs_contours_batch, say -- in one launch sequence with one
 * read-back; its point list and chain table go through cvs_chain_polylines and cvs_chain_measures as they are (neither needs an image, and
 * neither reads `reserved`), and through cvs_chain_refine_batch, which finds the plane of every point in the range table. */

/* EXTENSION: cvs_contour_chains for n >= 1 masks of the handle's image size at once.  masks: f32 or CVS_DEPTH_U8 planes (they may differ in
 * depth), pitched or dense, at one constant stride or not, ALL on the device or ALL on the host; foreground as in cvs_label.
 * The result is the concatenation over z = 0 .. n - 1 of what cvs_contour_chains writes for masks[z] alone: (x, y) are coordinates inside
 * the plane, chains[c].start is global -- the running sum of the lengths over all planes --, and chains[c].reserved is the plane z (a table
 * of cvs_contour_chains itself keeps 0 there).  Stated on its own: with LIN(z, p) = z * rows * cols + lin(p), links, nodes, chains,
 * direction and order are those of the cvs_contour_chains contract with LIN in place of lin, and no link joins pixels of different planes.
 * The chains and the points of a plane are therefore contiguous ranges: ranges[2 * z] is the index of the first chain of plane z,
 * ranges[2 * z + 1] that of its first point, entry n holds the totals, and an empty plane repeats its successor's pair (2 * (n + 1) ints).
 * points, chains and ranges are all in host or all in device memory (mem), whatever memory the masks are in.  *n_points and *n_chains
 * (both required) are always set; when either exceeds its capacity the call returns CVS_E_SIZE and writes no point, no chain and no range
 * (points = chains = ranges = NULL with both capacities 0 sizes the buffers).  ranges is written by every call that passes it and fits.
 * One read-back per call -- the four counters every size follows from --, whatever n is: synchronises the handle's stream,
 * CVS_E_UNSUPPORTED while it is being captured, CVS_E_STATE before the first setup.  CVS_E_SIZE: a plane of another size, or
 * n * rows * cols > 2^28 (32 frames x 3 maps x 1920 x 1080 = 199 065 600 fits).  CVS_E_BADARG: n < 1, masks of mixed memory, a NULL array
 * with a capacity > 0, a negative capacity, a pointer not aligned to 4 bytes, ranges NULL with a capacity > 0, an output that overlaps a mask
 * or another output.  Nothing is written when an argument is rejected.
 * The launch sequence depends on (rows, cols, n), on whether the planes lie at one constant stride (an [N, H, W] block, staged host
 * planes: addressed arithmetically) or not (a device table that launches fill from their arguments, 16 planes each), and on ceil(log2) of
 * the number of directed links -- never on what the masks hold.  The planes are labelled as one stacked block of n * rows rows that no
 * link and no union crosses a seam of, so every launch but the links, the labelling, the table and the emit is that of cvs_contour_chains
 * on that block.
 * Device memory: 10 bytes per pixel of ALL n planes and 24 bytes per directed link, in the handle scratch of cvs_contour_chains (grown
 * only, freed by cvs_destroy) -- 2.0 GB before the links for the 96 masks of 32 frames of 1920 x 1080. */
int cvs_contour_chains_batch(cvs_handle h, int n, const cvs_plane* masks,
                             int32_t* points, int point_capacity,     /* (x, y) int32 pairs, plane-local */
                             cvs_chain* chains, int chain_capacity,   /* start global, reserved = plane */
                             int32_t* ranges,                         /* 2 * (n + 1) ints */
                             int mem,                                 /* CVS_MEM_HOST / CVS_MEM_DEVICE: the three arrays */
                             int* n_points, int* n_chains);           /* both required, always set */

/* EXTENSION: cvs_chain_refine for the point list of cvs_contour_chains_batch.  maps: frames * n_maps (n_maps in 1..3) f32 planes of the
 * handle's image size, frame-major -- the UN-THINNED responses the masks came from; theta: `frames` planes, or NULL = the CVS_PLANE_THETA
 * state plane of frames 0 .. frames - 1 of the last cvs_pipeline_batch, as in cvs_nonmax_batch (CVS_E_STATE if the handle holds fewer
 * frames, or no orientation state).  ranges: the table cvs_contour_chains_batch wrote for n = frames * n_maps planes.
 * Per point i: the cvs_chain_refine contract, operation for operation, on plane z(i) = the largest z in 0 .. n - 1 with
 * ranges[2 * z + 1] <= i; the samples come from maps[z], theta from theta[z / n_maps].  Every xy and strength value is bit for bit that of
 * cvs_chain_refine(maps[z], theta[z / n_maps]) on the points of plane z.
 * points, ranges, xy and strength (may be NULL) are all in host or all in device memory (mem).  One launch, one lane per point; nothing
 * is read back: asynchronous and capturable with device arrays and device planes (planes at no constant stride need a descriptor table
 * in handle scratch; under capture that scratch must already have its size, which the same call made once eagerly sees to -- otherwise
 * CVS_E_UNSUPPORTED, and the handle works on).  Host arrays and host planes are staged, the call synchronises, and it is refused during
 * capture.
 * Device data is trusted for its meaning only: z(i) comes from a binary search that cannot leave 0 .. n - 1 whatever `ranges` holds,
 * coordinates are compared with cols / rows (unsigned) before any load, and a point outside the image stores NaN in xs, ys and strength
 * and reads no plane -- so no load leaves a plane.  A HOST ranges whose point column is not non-decreasing from 0 to n_points, and a
 * HOST point outside the image: CVS_E_BADARG before anything is queued.  CVS_E_BADARG as well: frames < 1, n_maps outside 1..3, maps NULL;
 * every other error as in cvs_chain_refine (points, ranges or xy NULL with n_points > 0 included).  n_points == 0: CVS_OK, nothing
 * queued.  Nothing is written when an argument is rejected. */
int cvs_chain_refine_batch(cvs_handle h, int frames, int n_maps,
                           const cvs_plane* maps,      /* frames * n_maps f32 planes, frame-major */
                           const cvs_plane* theta,     /* frames planes, or NULL */
                           const int32_t* points, int n_points,
                           const int32_t* ranges,      /* as cvs_contour_chains_batch writes it, n = frames * n_maps */
                           float* xy, float* strength, int mem);

/* the whole caller sequence of test/test.cpp:85-90 / example/steer.cpp:86-90 for one image:
 * setup(FULL) -> steer(theta_dom, g2,h2,e,mag,phase) -> find*(mag|e, phase).
 * outs[8] = {g2, h2, e, magnitude, phase, edges, dark, bright}; any entry may be NULL.
 * G4 with CVS_OPT_G4_EXTENSIONS = 1 (EXTENSION beyond the reference): the same for the G4/H4 bank, outs[8] = {g4, h4, e,
 * magnitude, phase, edges, dark, bright} -- every value bit-identical to cvs_setup(FULL) -> cvs_steer_map(NULL, ...) ->
 * cvs_find(magnitude | e, phase) on the same handle, the state afterwards that of cvs_setup(FULL) (or none, with
 * CVS_OPT_PERSIST_STATE = 0).  Two launches: the G4 pair launch of the basis planes, then one per-pixel pass over them.
 * G4 without the option: CVS_E_UNSUPPORTED. */
int cvs_pipeline(cvs_handle h, const cvs_plane* image, const cvs_plane* const outs[8]);
/* 8-bit outputs (cvs_pipeline, cvs_pipeline_batch): an output plane with mem = CVS_MEM_DEVICE | CVS_DEPTH_U8 or CVS_MEM_HOST |
 * CVS_DEPTH_U8 receives bytes (`step` in bytes, >= cols) -- what the reference's callers write to their files (example/steer.cpp:92-104,
 * test/test.cpp:92-94).  Any of the 8 outputs may be 8-bit, mixed with f32 ones; in a batch, output k has the same depth in every
 * frame.  Every byte equals the f32 call followed, per plane, by cvs_normalize_u8 (gain 0, the default: each map of each frame
 * normalised to its own min / max) or cvs_convert_u8(plane, gain, 0) (cvs_set_u8_gain > 0).  The state afterwards is that of the f32
 * call.  The three-maps launch (edges, dark, bright as bytes, CVS_OPT_PERSIST_STATE = 0, find on magnitude, the compatible arctangent,
 * G2, device planes) quantises in the filter launch (gain) or reduces min / max there and adds one quantise launch (normalise);
 * every other call composes the f32 maps with the quantise kernels (cvs_launch_info.u8_out says which). */
/* how cvs_pipeline / cvs_pipeline_batch make 8-bit outputs: gain 0 (default) = normalize(0, 255, NORM_MINMAX, CV_8UC1) per map
 * (example/steer.cpp:98-104), gain > 0 = convertTo(CV_8UC1, gain) (steer.cpp:92-97); negative or NaN: CVS_E_BADARG */
int cvs_set_u8_gain(cvs_handle h, float gain);
int cvs_get_u8_gain(cvs_handle h, float* gain);

/* The batch axis (example/steer.cpp:69-124,169: one independent pipeline per file): cvs_pipeline for
 * n images of identical size in ONE kernel launch (grid.z = frame; G4 with CVS_OPT_G4_EXTENSIONS = 1: one pair launch per
 * frame, then ONE per-pixel launch over all frames -- f32 device frames whose outputs lie at one constant frame stride).  outs is a flat array of n*8
 * planes, frame-major, order {g2,h2,e,magnitude,phase,edges,dark,bright}; an entry with data == NULL
 * is not written (outs == NULL: state only).  The state of every frame is kept; cvs_select_frame
 * picks the frame that cvs_state_plane / cvs_read_state / cvs_steer_* address (default 0).
 * Host planes, images too small for the fused kernel or non-default taps are processed frame by
 * frame with the same results. */
int cvs_pipeline_batch(cvs_handle h, const cvs_plane* images, int n, const cvs_plane* outs);
int cvs_select_frame(cvs_handle h, int frame);
int cvs_num_frames(cvs_handle h, int* n);

/* One Gaussian-pyramid level (BASELINE config 3; absent from the reference): cv::pyrDown
 * semantics -- 5-tap [1 4 6 4 1]/16 separable blur, BORDER_REFLECT_101, every second pixel.
 * dst must be ((rows+1)/2) x ((cols+1)/2). */
int cvs_pyr_down(cvs_handle h, const cvs_plane* src, const cvs_plane* dst);
/* cvs_setup(h, image, flags) and cvs_pyr_down(h, image, next_level) in ONE pass over the image ("filter this
 * pyramid level and make the next one", BASELINE config 3): the basis kernel emits the decimated level from
 * the rows it has staged for SteerableFiltersG2::setup (G2.cpp:62-68) anyway, so the image is read once instead
 * of twice.  Values are identical to the two separate calls; G4 handles, non-default widths, host planes and
 * planes of 2 GiB and more take the two launches internally. */
int cvs_setup_pyr(cvs_handle h, const cvs_plane* image, unsigned flags, const cvs_plane* next_level);

/* BASELINE config 3 in one call: `levels` handles (one per pyramid level, same device and stream), the level-0 image, and
 * levels - 1 caller-owned planes that receive the pyramid levels 1 .. levels-1 (sizes as for cvs_pyr_down).  The chain
 * cvs_setup_pyr(hs[0], image, ..), cvs_setup_pyr(hs[1], level 1, ..), ..., cvs_setup(hs[levels-1], last level): every level
 * image is read once (the filter launch of a level writes the next one).  Afterwards handle l holds the state of level l. */
int cvs_pyramid_setup(cvs_handle* hs, int levels, const cvs_plane* image, unsigned flags, const cvs_plane* level_images);

/* per-image min/max (cv::normalize NORM_MINMAX, test.cpp:92-94 / steer.cpp:96-98) and the
 * 8-bit quantise that follows; dst is rows*cols bytes with dst_step bytes per row. */
int cvs_normalize_u8(cvs_handle h, const cvs_plane* src, uint8_t* dst, size_t dst_step, int dst_mem);
/* Mat::convertTo(dst, CV_8UC1, alpha, beta) -- the `--gain` branch of example/steer.cpp:92-97 */
int cvs_convert_u8(cvs_handle h, const cvs_plane* src, float alpha, float beta, uint8_t* dst, size_t dst_step, int dst_mem);
/* the same for n planes in one go (a driver turning a whole block of feature maps into 8-bit files, steer.cpp:92-122 per
 * file): equally sized device planes at a constant stride take one min/max launch and one quantise launch for all of them;
 * anything else goes plane by plane.  dst[i] receives plane i.  HOST destinations: the bytes come down behind the launches and the
 * call synchronises once (plane by plane: once per plane).  DEVICE destinations (and device sources): nothing is read back, the call
 * is asynchronous on the handle's stream like the single-plane forms above. */
int cvs_normalize_u8_batch(cvs_handle h, const cvs_plane* src, int n, uint8_t* const* dst, size_t dst_step, int dst_mem);
int cvs_convert_u8_batch(cvs_handle h, const cvs_plane* src, int n, float alpha, float beta, uint8_t* const* dst, size_t dst_step, int dst_mem);

/* ---------------- the batch axis over the GPUs of one node (cvs_batch.cpp) ----------------
 * example/steer.cpp:169 runs cv::parallel_for_(Range(0, N), body): one independent SteerableFiltersG2 pipeline per
 * file (steer.cpp:69-124).  Here frame f of F belongs to rank floor(f * G / F) (contiguous blocks), every rank runs
 * cvs_pipeline_batch on its block -- no collective on the data path -- and RCCL moves data only at the edges.
 * A world is formed either by ONE process driving several devices (cvs_batch_create_local: ncclCommInitAll; a
 * device listed twice = rehearsal on a smaller box, transport = device copies instead of RCCL) or by one process per
 * GPU (cvs_batch_unique_id on one rank, the 128 bytes distributed by the caller, cvs_batch_create_rank everywhere).
 * Every rank of the world calls cvs_batch_run / cvs_batch_pyramid_setup with the same arguments; ranks that do not
 * hold the root pass NULL planes.  Calls return when the root holds the results.
 * In a world of several processes the ranks first AGREE (one 4-int ncclAllReduce, before any data is queued) that
 * every one of them can run the call -- the root's planes are what the call needs, every rank's staging fits, all ranks
 * were given the same geometry -- and otherwise all of them return an error with nothing queued; no rank is left
 * waiting in a receive.  (A failure after that point -- a kernel launch error on one rank -- is not recoverable across
 * processes: destroy the batch.)  An RCCL group that was started is always ended, also on errors. */
typedef struct cvs_batch_context* cvs_batch;
enum { CVS_BATCH_ID_BYTES = 128 };
enum { CVS_BATCH_TRANSPORT_NONE = 0, CVS_BATCH_TRANSPORT_RCCL = 1, CVS_BATCH_TRANSPORT_COPY = 2 };

typedef struct cvs_batch_cfg {
    int32_t rows, cols;          /* size of every frame */
    int32_t n_frames;            /* frames in the batch (all of them, on the root) */
    uint32_t outputs;            /* bit k = pipeline output k is wanted: g2,h2,e,magnitude,phase,edges,dark,bright */
    int32_t root;                /* rank that holds the inputs and receives the outputs */
    int32_t gather;              /* 1 = outputs are gathered on the root; 0 = they stay on the ranks (cvs_batch_local_result) */
    int32_t self_via_transport;  /* tests: the root's own block also travels through send / recv */
} cvs_batch_cfg;

typedef struct cvs_batch_timing {  /* HIP-event times on the ranks' streams, maximum over this process's ranks */
    double scatter_ms, compute_ms, gather_ms;
} cvs_batch_timing;

int cvs_batch_create_local(int kind, int width, float spacing, int ndev, const int* devices, cvs_batch* out);
int cvs_batch_unique_id(void* id128);
int cvs_batch_create_rank(int kind, int width, float spacing, const void* id128, int world, int rank, int device, cvs_batch* out);
int cvs_batch_destroy(cvs_batch b);
const char* cvs_batch_last_error(cvs_batch b);
int cvs_batch_info(cvs_batch b, int* world, int* nlocal, int* transport);
/* cvs_set_option on every engine of the batch (e.g. CVS_OPT_PERSIST_STATE = 0: outputs only; CVS_OPT_G4_EXTENSIONS = 1: a G4
 * batch runs the G4 caller pipeline of cvs_pipeline -- without it cvs_batch_run on a G4 batch is CVS_E_UNSUPPORTED) */
int cvs_batch_set_option(cvs_batch b, int option, int value);
/* BASELINE config 4 -- the loop of example/steer.cpp:169 over the node: inputs = n_frames dense f32 device planes on the
 * root, outputs = n_frames * 8 planes on the root, frame-major, order of cvs_pipeline (entries not selected by
 * cfg->outputs are ignored).  scatter (grouped ncclSend/ncclRecv) -> one cvs_pipeline_batch launch per rank ->
 * gather (grouped ncclSend/ncclRecv).  The root's own block is processed in place.
 * HOST planes (what the example holds: cv::Mat, steer.cpp:73-104; rows may be padded): inputs and requested outputs all
 * CVS_MEM_HOST; the inputs may be 8-bit (all of them CVS_MEM_HOST | CVS_DEPTH_U8, step in bytes: a quarter of the upload).  Nothing passes through the root's GPU then -- every rank uploads ITS frames from the caller's planes over
 * its own host link and downloads its outputs the same way, all ranks at once, upload / launch / download overlapped
 * chunk by chunk inside a rank.  Needs every rank in the calling process (cvs_batch_create_local, or a world of 1);
 * CVS_E_UNSUPPORTED otherwise.  timing: scatter = upload, gather = download, compute = the slowest rank's whole span.
 * The requested HOST outputs may be 8-bit planes as well (all of them CVS_MEM_HOST | CVS_DEPTH_U8, step in bytes) -- what the
 * example writes (steer.cpp:92-122): every map is then turned into bytes on the device, normalize(0, 255, NORM_MINMAX,
 * CV_8UC1) per map (steer.cpp:98-104) or convertTo(CV_8UC1, gain) (steer.cpp:92-97) as set by cvs_batch_set_u8_gain, chunk by
 * chunk behind the pipeline launch, and only bytes come back while the next chunk is uploaded and filtered. */
int cvs_batch_run(cvs_batch b, const cvs_batch_cfg* cfg, const cvs_plane* inputs, const cvs_plane* outputs, cvs_batch_timing* timing);
/* 8-bit host outputs of cvs_batch_run: gain = 0 (default) normalises every map to its own min / max (the example without
 * --gain, steer.cpp:98-104), gain > 0 is Mat::convertTo(CV_8UC1, gain) (steer.cpp:92-97) */
int cvs_batch_set_u8_gain(cvs_batch b, float gain);
/* after a run with gather = 0 (or on a non-root rank): this rank's block, [n_frames][n_planes][rows][cols] dense */
int cvs_batch_local_result(cvs_batch b, int rank, float** data, int* n_frames, int* n_planes, int* rows, int* cols);
/* BASELINE config 3 -- one large image and its Gaussian pyramid split over the ranks by rows: ncclBroadcast of the
 * image from the root, every rank builds the (cheap) pyramid and runs cvs_setup_rows on its band of every level, the
 * bands are gathered into the ROOT's state planes.  Afterwards cvs_batch_level hands out, on the root, one ordinary
 * handle per level whose state (cvs_state_plane / cvs_read_state / cvs_steer_*) is complete -- bit-identical to a
 * single-GPU cvs_setup of that level. */
int cvs_batch_pyramid_setup(cvs_batch b, const cvs_plane* image, int rows, int cols, int levels, unsigned flags, int root,
                            cvs_batch_timing* timing);
int cvs_batch_level(cvs_batch b, int level, cvs_handle* h, cvs_plane* level_image);

#ifdef __cplusplus
}
#endif
#endif /* CVSTEER_HIP_H */
