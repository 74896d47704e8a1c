// frame_bb.hip -- the frame path for the realistic rigs (plain intrinsics -- one matrix for all cameras, or one per camera
// as a calibration gives them: frame_bb_calib_kernel, BBState's PERK --, <= 16 cameras, <= 64 blobs per
// camera, <= 255 roots): epipolar correspondence search + EXACT branch-and-bound selection, one 256-lane workgroup per
// frame, persistent, everything between the blob arrays in and the kept points out in LDS (but the winners' points: phase E).  Replaces
//   find_point_correspondance_and_object_points   (reference computer_code/api/helpers.py:339-421)
// like frame_kernel.hip does (which keeps the general case: intrinsics that are not plain, wide frames, tiny frames, and
// the exhaustive walk every result of this file is tested against, MOCAP_EVAL_BB=0).
//
// What is different from frame_kernel.hip (measurements: DESIGN.md 3.1, docs/HISTORY.md):
//  * its own kernel and LDS layout: C <= 16 (blob indices of a group in one or two 64-bit words), any K_max <= 255 that fits
//    LDS -- the reference seam's default K_max = min(C M, 64) and the re-submit's C M included.
//  * phase B without the per-camera barrier chain.  The reference matches camera after camera (helpers.py:359-406) because a
//    blob no root claims becomes a new root for the cameras after it.  Only THAT is sequential: the camera-0 roots' lines,
//    gates, orders and claims in all other cameras are independent -> one barrier-free pass over (root, camera) pairs, then
//    the same pass for the provisional roots, then a chain over the cameras that is bookkeeping only.
//  * written for instruction issue, which is what binds it: one lane per (root, camera) pair with the camera's blobs walked
//    serially; the camera count (8) and, for 8 x 16 with K_max <= 48 / <= 64, the whole LDS layout at compile time; the
//    blocks' bounds cached between seed and test pass (one float each), their blob bytes and matrices built from what the
//    root's blocks share (pkbase); the camera tables behind one base pointer.
//  * a software pipeline over the frames: frame k + 1 is pulled from the queue and fetched straight into a spare LDS
//    buffer (global_load_lds, no registers) while frame k is searched.
//  * one evaluation path: a frame below the search threshold (MOCAP_BB_MIN_G, default 0 = never) queues all its blocks
//    unconditionally and takes the same evaluation rounds -- no second copy of the geometry core in the kernel.
//
// Phases per frame (256 lanes = 4 waves):
//   A   the prefetched frame becomes the current one (buffer swap)
//   B0  roots of camera 0; every (camera-0 root, camera) pair on its own lane: epipolar line (helpers.py:362-364),
//       the camera's blobs walked serially -- point-line distance (helpers.py:373), 5 px gate (helpers.py:375,383), hits
//       as a bit mask, written in stable (distance, index) order by repeated minimum (helpers.py:384), claim of the
//       closest hit BY VALUE (helpers.py:391) as a mask; speculative lines of every blob that might become a root
//   B1  wave 0: for camera i = 1 .. C-1: the roots created at cameras < i against camera i (lanes = (root, blob) groups
//       of 2^ceil(log2 M), ballots), then the unclaimed blobs of camera i become roots (helpers.py:402-406); meanwhile
//       waves 1-3 tabulate the DLT contribution of every blob (mocap_device.hpp dlt_contribution), one lane pulls the
//       next frame from the queue
//   C   per-root candidate counts (helpers.py:394-400), offsets, output slots (wave scans)
//   D   branch and bound over blocks of the Cartesian product: seeds, block tests, evaluation of the
//       survivors' candidates spread over all lanes; per (wave, root) slot = lexicographic minimum of (error bits,
//       candidate index) = np.argmin's first minimum (helpers.py:418) whatever the evaluation order
//   E   one lane per kept root: merge the four waves' slots, fetch the winning slot's record -- the point and the group's packed
//       blob bytes, left in the workgroup's L2-resident workspace by the lane that evaluated the candidate --, write xyz / err
//       and the corr row built from the bytes.  Reads slot_key / slot_g / outslot and nothing of the matching's state
#include "mocap_device.hpp"
#include "kernels.hpp"
#include <cstdlib>
#include "frame_common.hpp"
#include "bb_fold.hpp"
// (Round 6: the timing-only switches -- phases compiled out, parts run twice -- and the probe scheme, measured slower in
// round 5, left this file; they are in the history at 7c94a55 and in docs/HISTORY.md.  What remains switchable is what a
// test uses: -DMOCAP_DEBUG_EIGCHECK, the self-check build of tests/test_gpu_bb_adversarial.py.)

namespace mocap {

constexpr int kBBThreads = 256;
constexpr int kBBWaves = kBBThreads / 64;
constexpr int kBBRecs = kBBThreads + 64;  // surviving blocks queued between two evaluation rounds (flush above 64)
// a winner's record in the workgroup's workspace: the point (three doubles) + the group's packed blob bytes (CW words)
// words of packed blob bytes per group (Packed<CW>): one up to eight cameras, two up to sixteen -- the kernels' CW (BB_PICK), the
// LDS layout's and the records' all come from here
constexpr int bb_cw(int C) { return C <= 8 ? 1 : 2; }
constexpr uint32_t bb_rec_bytes(int CW) { return 24u + 8u * (uint32_t)CW; }
// a group's bytes are table rows (BBState::ROWS) where the whole layout is a compile-time constant and C ML + 1 rows fit a byte;
// ML a power of two: phase E takes the blob index back as byte & (ML - 1)
constexpr bool bb_group_rows(int CT, int ML, int RL) { return CT > 0 && ML > 0 && RL > 0 && CT * ML < 0xFF && (ML & (ML - 1)) == 0; }

// LDS carving, identical on host (size) and device (pointers): the frame's persistent state (blobs, per-blob DLT table,
// roots, hit lists), the search's arrays (block records, result slots -- dead while matching, which keeps its speculative
// lines there), the spare blob buffer of the frame pipeline and the cache of block bounds.
// Workgroups (= waves per SIMD) per CU an instantiation is built for: its register budget (512 / n per lane) and the occupancy
// step its LDS layout sizes the block cache for.  Four everywhere (128 VGPRs; 33-40 KB of LDS) except the 8-camera, 16-blob,
// 48-slot layout -- the bench's -- whose 29.2 KB leave room for FIVE frames per CU: 96 VGPRs (52 spilled instead of 22, +6 % per
// frame) and a block cache of 161 entries instead of 385, and still 4.50 -> 4.31 ms per 100 k frames (profiles/r06_wide_experiments.txt, (15)).
constexpr int bb_wg_per_cu(int RL) { return RL == 48 ? 5 : 4; }
constexpr size_t kBBCacheEntry = 4;  // bytes per cached block bound
constexpr int kBBLdsSlack = 1024;  // (measured: 512 keeps the occupancy step as well, 0 does not)
struct BBLayout {
  size_t bxy, bxy_nx, cnt_nx, bt, rbound, seedkey, slot_key, claimw, recs, rpk, scr, scr_bytes, goff, gcnt, outslot, boff, bnb, seedgh, slot_g, cnt,
      misc, bpl, nh, hits, act, root_blob, root_cam, nact, bnl, bv, pkbase, seen, bcache, total;
  int ncache;
  __host__ __device__ static size_t al(size_t x, size_t a) { return (x + a - 1) / a * a; }
  // row_words (the layouts fixed at compile time, 8 cameras: BBState::ROWS): a root's rows of nh and act are eight bytes at a
  // multiple of eight -- the search and phase C read a row as ONE word (the few bytes come out of the block cache)
  __host__ __device__ BBLayout(int C, int M, int R, int CW, int wg_per_cu, bool row_words = false) {
    size_t o = 0;
    auto take = [&](size_t bytes, size_t a) {
      o = al(o, a);
      const size_t at = o;
      o += bytes;
      return at;
    };
    // the two blob buffers come first: global_load_lds addresses LDS through M0, keep its targets in the low 64 KB
    bxy = take(sizeof(float2) * (size_t)C * M, 16);
    bxy_nx = take(sizeof(float2) * (size_t)C * M, 16);  // the NEXT frame's blobs land here while this one is searched
    cnt_nx = take(4 * (size_t)C, 4);
    bt = take(sizeof(double) * 10 * ((size_t)C * M + 1), 16);  // DLT contribution per (camera, blob): five b128 reads; + one record of zeros ("camera not in the group")
    rbound = take(8 * (size_t)R, 8);
    claimw = take(8 * (size_t)C, 8);
    pkbase = take(8 * (size_t)CW * R, 8);  // per root: its own blob and its single-hit cameras' blobs (phase C -> block_pk)
    // the search's block records and result slots: dead while matching -> phase B keeps the speculative epipolar
    // lines here (match(): lines of every blob that MIGHT become a root, computed off the critical path)
    scr = seedkey = take(8 * (size_t)R, 8);
    slot_key = take(8 * (size_t)kBBWaves * R, 8);
    recs = take(8 * (size_t)kBBRecs, 8);
    rpk = take(8 * (size_t)kBBRecs * CW, 8);
    seedgh = take(4 * (size_t)R, 4);
    slot_g = take(4 * (size_t)kBBWaves * R, 4);
    scr_bytes = o - scr;
    goff = take(4 * (size_t)(R + 1), 4);
    gcnt = take(4 * (size_t)R, 4);
    outslot = take(4 * (size_t)R, 4);
    boff = take(4 * (size_t)(R + 1), 4);
    bnb = take(4 * (size_t)R, 4);
    cnt = take(4 * (size_t)C, 4);
    misc = take(4 * 16, 4);
    bpl = take(2 * (size_t)R, 2);
    seen = take(2 * (size_t)R, 2);  // per root: the cameras it sees, one bit each (per-camera K: a view's position)
    nh = take((size_t)R * C, row_words ? 8 : 1);
    hits = take((size_t)R * C * M, 1);
    act = take((size_t)R * C, row_words ? 8 : 1);
    root_blob = take((size_t)R, 1);
    root_cam = take((size_t)R, 1);
    nact = take((size_t)R, 1);
    bnl = take((size_t)R, 1);
    bv = take((size_t)R, 1);
    // cache of the blocks' bounds (seed pass -> test pass: ONE float per block, bb_fold.hpp): as many entries as fit below
    // the next occupancy step of the 160 KB LDS (5, 4, 3, ... workgroups per CU), at most 1024
    // (rounds 5-9: {s1, trace} + the block's blob indices, 8 + 8 CW bytes -- 161 entries at five workgroups per CU, fewer than
    // the blocks of every third bench frame; the few blocks that survive rebuild their indices from pkbase, block_pk)
    bcache = take(0, 4);
    ncache = 0;
    const size_t per_entry = kBBCacheEntry;
    for (int per_cu = wg_per_cu; per_cu >= 1; per_cu--) {
      const size_t lim = ((size_t)160 * 1024 / per_cu - kBBLdsSlack) / 256 * 256;  // (slack: allocation granule, other LDS users)
      if (lim >= o + per_entry * 64) {
        const size_t n = (lim - o) / per_entry;
        ncache = (int)(n > 1024 ? 1024 : n);
        break;
      }
    }
    o += per_entry * (size_t)ncache;
    total = al(o, 16);
  }
};

// Root slots the launch lays out for a frame shape: the 8-camera, 16-blob shape has instantiations with the whole
// layout fixed at compile time (48 or 64 slots, 0 = none applies); every other shape is laid out for K_max itself.
static int bb_fixed_slots(int C, int M, int R) {
  const char* e = getenv("MOCAP_BB_FIXED_LAYOUT");  // 0: the runtime-layout instantiation for every shape (tests, A/B timing)
  if (e && e[0] == '0') return 0;
  if (C == 8 && M == 16 && R <= 48) return 48;
  if (C == 8 && M == 16 && R <= 64) return 64;
  return 0;
}
static int frame_bb_root_slots(int C, int M, int R) {
  const int f = bb_fixed_slots(C, M, R);
  return f ? f : R;
}
size_t frame_bb_lds_bytes(int C, int M, int R) { return BBLayout(C, M, frame_bb_root_slots(C, M, R), bb_cw(C), bb_wg_per_cu(bb_fixed_slots(C, M, R)), bb_fixed_slots(C, M, R) != 0).total; }
static size_t frame_bb_lds_bytes_min(int C, int M, int R) {
  const BBLayout L(C, M, frame_bb_root_slots(C, M, R), bb_cw(C), bb_wg_per_cu(bb_fixed_slots(C, M, R)), bb_fixed_slots(C, M, R) != 0);
  return L.total - kBBCacheEntry * (size_t)L.ncache;
}
bool frame_bb_fits(int C, int M, int R) {
  // blob indices and root numbers are bytes (0xFF = none); a (root, blob) group is at most one wave; the expanded
  // candidate list of one evaluation round is counted in 22 bits (FrameArgs::bb_pl is lowered by the host if needed)
  return C >= 2 && C <= 16 && M >= 1 && M <= 64 && R >= 1 && R <= 255 && frame_bb_lds_bytes_min(C, M, R) <= (size_t)128 * 1024;
}

// blob indices of one (partial) group: one byte per camera, NONE = the camera is open or not in the group.  Runtime layouts:
// the byte is the blob index, NONE = 0xFF.  Fixed layouts (bb_group_rows): the byte is the blob's ROW c ML + k of the per-blob
// table -- what every consumer of a group needs (the DLT record at bt + 80 row, the observation at bxy[row]) --, NONE = C ML, the
// table's record of zeros.
template <int CW, uint32_t NONE = 0xFFu>
struct Packed {
  unsigned long long w[CW];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < CW; k++) w[k] = NONE * 0x0101010101010101ull;
  }
  __device__ __forceinline__ void set(int c, uint32_t idx) {  // the camera's byte must still be NONE
    if (CW == 1)
      w[0] ^= (unsigned long long)(idx ^ NONE) << (8 * c);
    else
      w[c >> 3] ^= (unsigned long long)(idx ^ NONE) << (8 * (c & 7));
  }
  __device__ __forceinline__ uint32_t get(int c) const {
    return CW == 1 ? (uint32_t)(w[0] >> (8 * c)) & 0xFFu : (uint32_t)(w[c >> 3] >> (8 * (c & 7))) & 0xFFu;
  }
};

// CT: the camera count when it is known at compile time (8: the headline rig -- camera loops unroll, their control
// and address arithmetic leave the scalar unit, which the issue-bound kernel shares with the vector work), 0 = runtime
// The camera tables as ONE base pointer plus offsets fixed by the camera count (mocap_set_cameras lays its block out as
// Pq | RT | K4 | F, capi.hip; identical intrinsics: Pq is [C][12]; launch_frame_bb checks the pointers against this).
// Through a CamView the compiler re-read the four table pointers from the kernel arguments before every table read --
// per reprojected view: arguments -> RT -> arguments -> K4, four dependent scalar-cache round trips around 42 vector
// instructions.  The base is kept in registers (its value is hidden from the optimiser once, at the start of the
// kernel), so a view costs one round trip, and K4 (one entry: identical intrinsics) is read once per candidate.
// PERK (per-camera intrinsics, the calibrated rigs): Pq is [j][C][12] = K[j] [R|t][c] for j <= c (12 C C doubles), K4 has one
// entry per intrinsics index; the other tables follow at the offsets that gives.
template <int CT, bool PERK = false>
struct BBCamTables {
  const double* base;
  static constexpr int C = CT;
  static constexpr int kPq = PERK ? 12 * CT * CT : 12 * CT;
  __device__ __forceinline__ ctab_t pq(size_t off) const { return as_ctab(base + off); }
  __device__ __forceinline__ ctab_t rt(size_t off) const { return as_ctab(base + kPq + off); }
  __device__ __forceinline__ ctab_t k4(size_t off) const { return as_ctab(base + kPq + 12 * CT + off); }
  __device__ __forceinline__ const double* f() const { return base + kPq + 16 * CT; }
};
template <bool PERK>
struct BBCamTables<0, PERK> {
  const double* base;
  int C;
  __device__ __forceinline__ ctab_t pq(size_t off) const { return as_ctab(base + off); }
  __device__ __forceinline__ ctab_t rt(size_t off) const { return as_ctab(base + (PERK ? 12 * C * C : 12 * C) + off); }
  __device__ __forceinline__ ctab_t k4(size_t off) const { return as_ctab(base + (PERK ? 12 * C * C + 12 * C : 24 * C) + off); }
  __device__ __forceinline__ const double* f() const { return base + (PERK ? 12 * C * C + 16 * C : 28 * C); }
};

// Issue priority of the frame's phases (s_setprio: arbitration between the waves of one SIMD -- here the four frames
// of a CU, each with one wave per SIMD, each in a phase of its own).  The candidate evaluation is the bulk of the work and
// runs at 0; everything that holds the other waves of its workgroup at a barrier runs above it: the single-wave stretches
// (chain bookkeeping, scans) at 3, the rest of the matching and the output at 2, the seed pass at 1.  A frame's serial
// depth then costs what it costs alone, not what it costs sharing its SIMD's issue slots with three evaluations:
// 4.70 -> 4.50 ms per 100 k frames of 8 x 16 (profiles/r06_wide_experiments.txt, (14)).
enum { kPrioEval = 0, kPrioSeed = 1, kPrioPhase = 2, kPrioSerial = 3 };
template <int P>
__device__ __forceinline__ void bb_prio() {
  __builtin_amdgcn_s_setprio(P);
}

// A double rounded to float32 towards +inf (what __double2float_ru returns, for every input, in 7 instructions instead of 17): the
// nearest float, and where that lies below the value its upper neighbour -- one step in the bit pattern, up for a float >= +0, down
// for a negative one (-inf -> -FLT_MAX); a NaN or a value the nearest float does not lie below is kept.
__device__ __forceinline__ float f32_round_up(double v) {
  const float f = (float)v;
  const int32_t b = __float_as_int(f);
  return (double)f < v ? __int_as_float(b + ((b >> 31) | 1)) : f;
}

// ML, RL: the layout's blobs per camera and root slots when they are known at compile time (with CT: every LDS array
// sits at a constant address, which takes the base registers, their spills to vector lanes and the address arithmetic
// out of every phase -- 5.72 -> 5.39 ms per 100 k frames of 8 x 16), 0 = runtime.  ML is the frame's M_max itself (the
// blob buffers are copied flat); RL only has to hold K_max roots: the slot arrays are laid out for RL, the root limit
// and the output stride stay K_max.
// PERK: per-camera intrinsics (frame_bb_calib_kernel below).  The reference takes the intrinsics of a view by the POSITION of
// its camera among the cameras the group sees (helpers.py:305-307, :231-237); every candidate of a root sees the same cameras,
// so the position is a property of (root, camera): the running count of seen cameras in every ascending camera loop below.
// The per-blob DLT table holds the contribution at position = camera (K[c] with pose c: a camera-0 root seen by every camera
// before c, the common case); a view at a lower position (a camera before it saw nothing of the root, or the root was created
// at a later camera) takes dlt_contribution on Pq[position][camera] on the spot -- the same function on the same operands
// as the exhaustive walk's, hence the same bits, summed in the same ascending camera order.
template <bool F32R, int CW, int CT, int ML, int RL, bool PERK = false>
struct BBState {
  static constexpr int T = kBBThreads, W = kBBWaves;
  // Group bytes as table rows (Packed): the layouts fixed at compile time whose rows and the record of zeros fit a byte -- 8 x 16:
  // rows 0 .. 127, zeros at 128.  gbyte(c, k): blob k of camera c as a group's byte; grow(c, byte): its table row.
  static constexpr bool ROWS = bb_group_rows(CT, ML, RL);
  static constexpr uint32_t kNone = ROWS ? (uint32_t)(CT * ML) : 0xFFu;
  typedef Packed<CW, kNone> Pk;
  // Round 14, the same layouts: a root's row of nh and of act is ONE 64-bit word (BBLayout: row_words) -- the search's decodes
  // and phase C take a camera's hit count and a digit's camera from two registers by shift and mask instead of a chain of
  // dependent byte reads; the pair loop keeps the closest hit while it walks the blobs and orders the rest only.
  static_assert(!ROWS || (CT == 8 && CW == 1), "a row of nh / act as one word: eight cameras");
  __device__ __forceinline__ unsigned long long row_word64(const uint8_t* rows, int r) const { return ((const unsigned long long*)rows)[r]; }
  __device__ static __forceinline__ uint32_t byte_of(unsigned long long w, uint32_t k) { return (uint32_t)(w >> (8u * k)) & 0xFFu; }
  // The provisional roots listed once per frame (match(), behind stage 0's barrier): the fixed layouts whose blobs of a camera
  // fit the low half of a wave's lane mask (mbcnt_lo) and whose (camera, blob) numbers c ML + k fit a byte
  static constexpr bool PLIST = CT > 0 && ML > 0 && RL > 0 && ML < 32 && CT * ML <= 256 && (ML & (ML - 1)) == 0;
  __device__ __forceinline__ uint32_t gbyte(int c, uint32_t k) const { return ROWS ? (uint32_t)c * (uint32_t)ML + k : k; }
  __device__ __forceinline__ size_t grow(int c, uint32_t b) const { return ROWS ? (size_t)b : (size_t)c * M + b; }
  const FrameArgs& p;
  BBCamTables<CT, PERK> cv;
  const int C_, M, R, RS;  // R = K_max (root limit, output stride), RS = root slots of the layout
  int tid, lane, wave;
  // The lane's number taken afresh (an empty asm the optimiser cannot see through): what a phase derives from it -- LDS addresses,
  // (root, camera) pair indices, masks -- is computed in that phase instead of once before the frame loop, where it would sit in a
  // register for the whole frame, i.e. in scratch (Makefile: FRAME_BB_FLAGS has the measurements)
  __device__ __forceinline__ void fresh_tid() {
    int t = tid;
    asm volatile("" : "+v"(t));
    tid = t;
    lane = t & 63;
    wave = t >> 6;
  }
  __device__ __forceinline__ int cn() const { return CT > 0 ? CT : C_; }
  // Measuring build (-DMOCAP_BB_PHASE_CLOCKS, lib/libmocap_core_phaseclocks.so, scripts/time_frame_phases.py): wave 0 reads the
  // cycle counter behind the barriers that separate a frame's phases and keeps one 32-bit sum per phase (a workgroup's cycles of
  // one launch fit); the sums go to the counters behind the caller's status array when the workgroup leaves the frame loop
  // (frame_bb_body.inc), the way the self-check build hands over its counts.  The clocks cost registers and wave 0 its issue
  // slots: the figures are SHARES of a frame, not times.  Without the define pc_mark() is empty and every code object is,
  // instruction for instruction, what it is without this text.
  enum { PC_OTHER = 0, PC_PAIRS0, PC_PAIRS1, PC_B1_TABLE, PC_ROW_COPY, PC_PHASE_C, PC_SEED_PASS, PC_SEED_PUSH, PC_EVAL, PC_TEST, PC_PHASE_E, PC_COUNT };
#ifdef MOCAP_BB_PHASE_CLOCKS
  uint32_t pc_last = 0, pc_sum[PC_COUNT] = {};
  template <int PH>
  __device__ __forceinline__ void pc_mark() {
    if (__builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) == 0) {  // (wave-uniform: the counter and the sums stay scalar)
      const uint32_t now = (uint32_t)__builtin_readcyclecounter();
      pc_sum[PH] += now - pc_last;
      pc_last = now;
    }
  }
  __device__ __forceinline__ void pc_start() { pc_last = (uint32_t)__builtin_readcyclecounter(); }
  __device__ __forceinline__ void pc_flush() const {
    // (the caller's launch only: the status array of the re-submit's second pass, FrameArgs::n_frames_dev, is the library's own
    // and has the self-check builds' two spare slots)
    if (threadIdx.x == 0 && !p.n_frames_dev)
      for (int k = 0; k < PC_COUNT; k++) atomicAdd(&p.status[p.n_frames + k], (int)(pc_sum[k] >> 8));  // (units of 256 cycles: the grid's sum fits 31 bits)
  }
#else
  template <int PH>
  __device__ __forceinline__ void pc_mark() {}
  __device__ __forceinline__ void pc_start() {}
  __device__ __forceinline__ void pc_flush() const {}
#endif
  double* bt;
  float2 *bxy, *bxy_nx;
  int32_t* cnt_nx;
  unsigned long long *rbound, *seedkey, *slot_key, *claimw, *rpk;
  struct BRec { uint32_t gh, rs; };  // surviving block gh of root (rs & 0xFF); its candidates start at rs >> 8 of the expanded list
  BRec* recs;
  uint32_t *goff, *gcnt, *boff, *bnb, *seedgh, *slot_g;
  int32_t *outslot, *cnt, *misc;
  uint16_t* bpl;
  uint8_t *nh, *hits, *act, *root_blob, *root_cam, *nact, *bnl, *bv;
  float* bcache;       // [ncache] the first blocks' bounds, folded (BBLayout::bcache, bb_fold.hpp)
  unsigned long long* pkbase;  // [RS][CW] blob indices every block of the root shares
  uint16_t* seen;      // [RS] cameras the root sees
  int ncache;
  unsigned char* scr;  // phase B scratch = the search's records and slots (BBLayout::scr)
  size_t scr_bytes;
  static constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;

  __device__ BBState(const FrameArgs& p_, unsigned char* smem)
      : p(p_), C_(p_.cv.C), M(ML > 0 ? ML : p_.M), R(p_.K_max), RS(RL > 0 ? RL : p_.K_max), tid(threadIdx.x), lane(threadIdx.x & 63), wave(threadIdx.x >> 6) {
    const int C = cn();
    {
      const unsigned long long ta = (unsigned long long)(uintptr_t)p_.cv.Pq;
      uint32_t tlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ta);
      uint32_t thi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(ta >> 32));
      asm volatile("" : "+s"(tlo), "+s"(thi));
      cv.base = (const double*)(uintptr_t)(((unsigned long long)thi << 32) | tlo);
      if constexpr (CT == 0) cv.C = C;
    }
    const BBLayout L(C, M, RS, CW, bb_wg_per_cu(RL), ROWS);
    bt = (double*)(smem + L.bt);
    bxy = (float2*)(smem + L.bxy);
    bxy_nx = (float2*)(smem + L.bxy_nx);
    cnt_nx = (int32_t*)(smem + L.cnt_nx);
    rbound = (unsigned long long*)(smem + L.rbound);
    seedkey = (unsigned long long*)(smem + L.seedkey);
    slot_key = (unsigned long long*)(smem + L.slot_key);
    claimw = (unsigned long long*)(smem + L.claimw);
    recs = (BRec*)(smem + L.recs);
    rpk = (unsigned long long*)(smem + L.rpk);
    goff = (uint32_t*)(smem + L.goff);
    gcnt = (uint32_t*)(smem + L.gcnt);
    outslot = (int32_t*)(smem + L.outslot);
    boff = (uint32_t*)(smem + L.boff);
    bnb = (uint32_t*)(smem + L.bnb);
    seedgh = (uint32_t*)(smem + L.seedgh);
    slot_g = (uint32_t*)(smem + L.slot_g);
    cnt = (int32_t*)(smem + L.cnt);
    misc = (int32_t*)(smem + L.misc);
    bpl = (uint16_t*)(smem + L.bpl);
    nh = (uint8_t*)(smem + L.nh);
    hits = (uint8_t*)(smem + L.hits);
    act = (uint8_t*)(smem + L.act);
    root_blob = (uint8_t*)(smem + L.root_blob);
    root_cam = (uint8_t*)(smem + L.root_cam);
    nact = (uint8_t*)(smem + L.nact);
    bnl = (uint8_t*)(smem + L.bnl);
    bv = (uint8_t*)(smem + L.bv);
    scr = smem + L.scr;
    scr_bytes = L.scr_bytes;
    bcache = (float*)(smem + L.bcache);
    pkbase = (unsigned long long*)(smem + L.pkbase);
    seen = (uint16_t*)(smem + L.seen);
    ncache = L.ncache;
  }

  // ---------------------------------------------------------------- phase B building blocks
  // Epipolar line of root r in camera i: cv.computeCorrespondEpilines on a float32 point -- double math, scale by
  // 1/sqrt(a^2+b^2), float32 result (helpers.py:363-364); den = sqrt(a^2+b^2) of the ROUNDED line, by which
  // helpers.py:373 divides again, and its reciprocal for the quotients.  The same expressions, in the same order, as
  // frame_kernel.hip phase B1 (bit-identical by construction; tested against it).
  struct Line { double a, b, c, den, rden; };
  __device__ __forceinline__ Line epiline(int r, int i) const { return epiline_of(root_cam[r], root_blob[r], i); }
  __device__ __forceinline__ Line epiline_of(int rc, int rb, int i) const {
    const int C = cn();
    const double* Fm = cv.f() + 9 * ((size_t)rc * C + i);  // (per-lane camera pair: vector loads, L1/L2-resident table)
    const float2 rp = bxy[(size_t)rc * M + rb];
    const double x = (double)rp.x, y = (double)rp.y;
    double a = Fm[0] * x + Fm[1] * y + Fm[2];
    double b = Fm[3] * x + Fm[4] * y + Fm[5];
    double c = Fm[6] * x + Fm[7] * y + Fm[8];
    double nu = a * a + b * b;
    nu = nu != 0.0 ? 1.0 / sqrt(nu) : 1.0;
    a *= nu;
    b *= nu;
    c *= nu;
    if (F32R) {
      a = (double)(float)a;
      b = (double)(float)b;
      c = (double)(float)c;
    }
    Line L;
    L.a = a;
    L.b = b;
    L.c = c;
    L.den = sqrt(a * a + b * b);
    L.rden = recip_refined(L.den);
    return L;
  }

  // Gate / order / claim of up to 64 (root, camera) pairs whose lines sit in the lanes of this wave (lane l holds the
  // line of pair l; pair_r / pair_i = its root and camera, n_pairs valid).  Lanes regroup as (pair slot, blob):
  // GS = 2^gs_shift >= M lanes per pair, 64 / GS pairs per sub-pass.
  // CHAIN: every pair is in camera `cam` (wave-uniform, Mi blobs); the blobs the pairs claim come back as a mask
  // (wave-uniform) instead of going to claimw[] -- the chain over the cameras keeps its state in registers.
  template <bool CHAIN>
  __device__ __forceinline__ unsigned long long match_pairs(const Line& mine, int pair_r, int pair_i, int n_pairs, int gs_shift,
                                                            int cam = 0, int Mi_chain = 0) {
    const int C = cn();
    const int GS = 1 << gs_shift, PPS = 64 >> gs_shift;
    const int k = lane & (GS - 1), q = lane >> gs_shift;
    const int gl0 = lane & ~(GS - 1);
    const unsigned long long gall = gs_shift == 6 ? ~0ull : ((1ull << GS) - 1ull);
    unsigned long long claims = 0ull;
    for (int s0 = 0; s0 < n_pairs; s0 += PPS) {  // wave-uniform trip count
      const int src = s0 + q;                    // the lane that holds this group's line
      const bool has = src < n_pairs;
      const int sl = has ? src : 0;
      const double la = __shfl(mine.a, sl), lb = __shfl(mine.b, sl), lc = __shfl(mine.c, sl);
      const double lden = __shfl(mine.den, sl), lrden = __shfl(mine.rden, sl);
      const int r = __shfl(pair_r, sl);
      const int i = CHAIN ? cam : __shfl(pair_i, sl);
      const int Mi = has ? (CHAIN ? Mi_chain : cnt[i]) : 0;
      const bool valid = k < Mi;
      float2 pt = make_float2(0.f, 0.f);
      double d = 0.0;
      bool hit = false;
      if (valid) {
        pt = bxy[(size_t)i * M + k];
        const double num = fabs(la * (double)pt.x + lb * (double)pt.y + lc);  // helpers.py:373
        d = div_by(num, lden, lrden);
        hit = d < p.gate_px;  // strict <, helpers.py:375,383
      }
      const unsigned long long wm = __ballot(hit);
      const unsigned long long gm = (wm >> gl0) & gall;
      // rank among the group's hits by (distance, blob index): a stable order where NumPy's default argsort is not
      // (helpers.py:384; documented deviation).  The loop runs over the hits of the whole wave (a handful), each
      // broadcast from its lane; a lane counts the ones of its own group that precede it.
      int rank = 0;
      const unsigned int dlo = (unsigned int)__double_as_longlong(d), dhi = (unsigned int)(__double_as_longlong(d) >> 32);
      for (unsigned long long mm = wm; mm;) {
        const int j = __ffsll((long long)mm) - 1;  // wave-uniform
        mm &= mm - 1;
        const double dj = __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)dhi, j) << 32) |
                                               (unsigned int)__builtin_amdgcn_readlane((int)dlo, j));
        const bool mine_grp = (j & ~(GS - 1)) == gl0 && j != lane;
        rank += (hit && mine_grp && (dj < d || (dj == d && j < lane))) ? 1 : 0;
      }
      if (hit) hits[((size_t)r * C + i) * M + rank] = (uint8_t)gbyte(i, (uint32_t)k);
      const unsigned long long g0 = (__ballot(hit && rank == 0) >> gl0) & gall;
      // removal by value (helpers.py:391): every blob with the closest hit's coordinates is claimed
      bool same = false;
      if (valid && g0) {
        const float2 p0 = bxy[(size_t)i * M + (__ffsll((long long)g0) - 1)];
        same = pt.x == p0.x && pt.y == p0.y;
      }
      const unsigned long long cw = __ballot(same);
      if (CHAIN) {
        for (int sh = 0; sh < 64; sh += GS) claims |= (cw >> sh) & gall;  // lane -> blob: fold the groups onto each other
      }
      if (has && k == 0) {
        nh[(size_t)r * C + i] = (uint8_t)__popcll(gm);
        if (!CHAIN) {
          const unsigned long long cm = (cw >> gl0) & gall;
          if (cm) atomicOr(&claimw[i], cm);
        }
      }
    }
    return claims;
  }

  // The next frame's blobs and counts travel from HBM straight into the spare LDS buffer while the current frame is
  // searched (global_load_lds: no VGPR is held -- a register prefetch was spilled to scratch by the compiler, i.e. went
  // to HBM and back): neither the queue atomic nor the first touch of a frame sits on the per-frame critical path.
  // They are issued behind the matching and waited for at the search's entry (search(): the compiler waits for them before the
  // first LDS access that follows anyway -- it cannot tell their LDS target from any other address), so what they overlap is the
  // frame's bookkeeping stores and the other workgroups of the CU; a frame without candidates waits at its last barrier
  // (wait_own_stores: vmcnt(0) counts them).
  __device__ __forceinline__ void prefetch_lds(int64_t frame) const {
    const int C = cn();
    const float* src = p.blobs + (size_t)frame * C * M * 2;
    const int n_dw = C * M * 2;
    for (int base = wave * 64; base < n_dw; base += T)  // a wave writes 64 consecutive dwords at its LDS base + 4 lane
      if (base + lane < n_dw)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + base + lane),
                                         (__attribute__((address_space(3))) void*)((float*)bxy_nx + base), 4, 0, 0);
    if (wave == 0 && lane < C)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p.counts + (size_t)frame * C + lane),
                                       (__attribute__((address_space(3))) void*)cnt_nx, 4, 0, 0);
  }
  // the prefetched frame becomes the current one (buffer swap)
  __device__ __forceinline__ void stage(int64_t frame) {
    fresh_tid();
    const int C = cn();
    float2* t = bxy;
    bxy = bxy_nx;
    bxy_nx = t;
    if (tid < C) {
      const int n = cnt_nx[tid];
      cnt[tid] = n < 0 ? 0 : (n > M ? M : n);
      claimw[tid] = 0ull;
    }
    if (tid == 0) {
      misc[MI_STATUS] = 0;
      misc[MI_OMAX] = 0;
    }
  }

  // ---------------------------------------------------------------- phases B-C (the frame is staged)
  // Also pulls the NEXT frame from the queue into misc[MI_NEXT] (one lane of wave 1, while wave 0 walks the cameras: the
  // atomic's round trip to L2 is off everybody's critical path), so that every lane can prefetch that frame afterwards.
  __device__ void match() {
    fresh_tid();
    const int C = cn();
    __syncthreads();
    int gs_shift = 0;
    while ((1 << gs_shift) < M) gs_shift++;
    const int n0 = cnt[0] < R ? cnt[0] : R;
    {  // roots from camera 0 (helpers.py:349,357)
      for (int r = tid; r < n0; r += T) {
        root_cam[r] = 0;
        root_blob[r] = (uint8_t)r;
      }
      if (tid == 0 && cnt[0] > R) misc[MI_STATUS] |= MOCAP_ST_ROOT_OVERFLOW_;
    }
    __syncthreads();
    // B0: the (camera-0 root, camera) pairs, ONE LANE PER PAIR, the camera's blobs walked serially (the kernel is issue
    // bound: ~10 wave instructions per pair instead of ~250 per 4 pairs with a lane per (pair, blob)).  Pass 1 collects the
    // gated blobs of the pair as a bit mask (M <= 64); pass 2 extracts them in (distance, index) order by repeated minimum
    // (hit lists are a handful long; distances are recomputed: same expression, same bits).
    // Stage 1 of the same pass: the PROVISIONAL roots -- the blobs of cameras 1 .. C-1 the camera-0 roots left unclaimed
    // (only they can become roots, helpers.py:402-406) -- against the cameras after them, into staging rows (the search's
    // dead arrays); the chain over the cameras below then only decides which provisional roots are real.  A frame whose
    // provisional roots do not fit the staging rows (or one wave) takes the chain with its own matching, as before.
    auto U_of = [&](int j) {  // provisional blobs of camera j (valid behind stage 0's barrier)
      const int n = cnt[j];
      return ~claimw[j] & (n >= 64 ? ~0ull : ((1ull << n) - 1ull));
    };
    int n_prov = 0, n_ppairs = 0;
    bool pre = false;
    uint8_t* nh_s = nullptr;
    uint8_t* hits_s = nullptr;
    unsigned long long* pclaim = (unsigned long long*)scr;
    // PLIST: the provisional roots in (camera, blob) order, one byte j ML + k each, in act[] (written in phase C, read by the
    // search: dead while matching; C ML bytes at most, R C are there); p_end[j]: the pairs and the provisional roots of cameras
    // 1 .. j as one word, pairs << 16 | roots (both < 2^16: C ML blobs), in goff[] (phase C's scan writes it: dead as well).
    // In LDS rather than in registers: as wave-uniform values they cost the headline kernel 14 more scalar spills to vector lanes
    uint8_t* plist = act;
    uint32_t* p_end = goff;
    {
      int Mmax = 0;
      for (int c = 1; c < C; c++) Mmax = cnt[c] > Mmax ? cnt[c] : Mmax;  // wave-uniform
#pragma nounroll
      for (int stage_ = 0; stage_ < 2; stage_++) {
        const int stage = __builtin_amdgcn_readfirstlane(stage_);  // (opaque: one copy of the pair code)
        int NP = n0 * (C - 1);
        if (stage == 1) {
          // (explicit: the compiler emitted THIS barrier without the s_waitcnt lgkmcnt(0) every other one has -- a wave could
          // read the claim words while another wave's ds_or of stage 0 was still queued: provisional sets that differed between
          // waves, one wrong frame in ~10^5)
          block_sync_lds();  // the camera-0 roots' claims are complete
          pc_mark<PC_PAIRS0>();
          if constexpr (PLIST) {
            // behind this barrier the provisional roots are fixed: every wave lists them once -- a lane per blob of one camera
            // takes its rank from the camera's unclaimed mask and the running base, and leaves (camera, blob) in the list's slot
            // of that rank; all waves write the same bytes.  No lane walks the cameras or a mask's set bits afterwards.
#pragma unroll
            for (int j = 1; j < CT; j++) {
              const uint32_t U = ~((const uint32_t*)claimw)[2 * j] & ((1u << cnt[j]) - 1u);   // (cnt <= ML < 32; the same in every lane)
              if (lane < ML && ((U >> lane) & 1u)) plist[__builtin_amdgcn_mbcnt_lo(U, (uint32_t)n_prov)] = (uint8_t)(j * ML + lane);
              n_prov += __popc(U);
              n_ppairs += __popc(U) * (CT - 1 - j);
              if (lane == 0) p_end[j] = ((uint32_t)n_ppairs << 16) | (uint32_t)n_prov;
            }
            wave_lds_sync();
          } else
          for (int j = 1; j < C; j++) {
            const int np = __popcll(U_of(j));
            n_prov += np;
            n_ppairs += np * (C - 1 - j);
          }
          pre = n_prov <= 64 && (size_t)n_prov * C * (8 + 1 + (size_t)M) <= scr_bytes;
          if (!pre) break;
          nh_s = (uint8_t*)(pclaim + (size_t)n_prov * C);
          hits_s = nh_s + (size_t)n_prov * C;
          NP = n_ppairs;
        }
        for (int base = wave * 64; base < NP; base += W * 64) {
          const int pi = base + lane;
          const bool have = pi < NP;
          int r = 0, i = 1, Mi = 0;   // r: row the pair writes (stage 0: the root; stage 1: the provisional root's staging row)
          Line L = {0, 0, 0, 1, 1};
          if (have) {
            if (stage == 0) {
              r = pi / (C - 1);
              i = 1 + (pi - r * (C - 1));
              L = epiline(r, i);
            } else if constexpr (PLIST) {
              // the pair's camera: the first whose prefix of pair counts exceeds the pair's number (pi < n_ppairs = the pairs of p_end[C - 2]);
              // its provisional root by one division, the root's blob from the list
              int j = 1;
              uint32_t before = 0;  // pairs << 16 | roots of the cameras before the pair's
              const uint32_t key = ((uint32_t)pi << 16) | 0xFFFFu;  // key >= p_end[jj]  <=>  pi >= its pairs
              uint32_t pe[CT > 2 ? CT - 2 : 1];
#pragma unroll
              for (int jj = 1; jj <= CT - 2; jj++) pe[jj - 1] = p_end[jj];  // (independent reads at constant addresses)
#pragma unroll
              for (int jj = 1; jj <= CT - 2; jj++) {
                const bool ge = key >= pe[jj - 1];
                j += ge ? 1 : 0;
                before = ge ? pe[jj - 1] : before;
              }
              const uint32_t acc = before >> 16, pb = before & 0xFFFFu;
              uint32_t ord, off;
              divmod_tiny((uint32_t)pi - acc, (uint32_t)(CT - 1 - j), ord, off);  // (< 64 x 15, span <= 14)
              r = (int)(pb + ord);
              const int k = plist[r] & (ML - 1);
              i = j + 1 + (int)off;
              L = epiline_of(j, k, i);
            } else {
              int j = 1, acc = 0, pb = 0, span = C - 2;
              unsigned long long U = 0ull;
              for (; j <= C - 2; j++) {
                span = C - 1 - j;
                U = U_of(j);
                const int nj = __popcll(U) * span;
                if (pi < acc + nj) break;
                acc += nj;
                pb += __popcll(U);
              }
              uint32_t ord, off;
              divmod_tiny((uint32_t)(pi - acc), (uint32_t)span, ord, off);  // (< 64 x 15, span <= 14)
              for (uint32_t t = 0; t < ord; t++) U &= U - 1;
              const int k = __ffsll((long long)U) - 1;
              i = j + 1 + (int)off;
              r = pb + (int)ord;
              L = epiline_of(j, k, i);
            }
            Mi = cnt[i];
          }
          const float2* pts = bxy + (size_t)i * M;
          auto dist = [&](int k) {
            const float2 pt = pts[k];
            return div_by(fabs(L.a * (double)pt.x + L.b * (double)pt.y + L.c), L.den, L.rden);  // helpers.py:373
          };
          unsigned long long hm = 0ull;
          // (ROWS: the closest hit falls out of the walk -- ascending index, strict <: ties keep the smaller index, pass 2's rule)
          double bd0 = __builtin_huge_val();
          int bk0 = 0;
          if constexpr (ROWS) {
            // Round 15: no wait, branch or exact distance per blob.  All ML slots of the camera are read as words of two blobs,
            // whatever the count (slots at or beyond it hold the caller's bytes: the count mask below keeps them out of cand, hence
            // out of hm, the minimum and the claim); with the float32 line the wide variant's pre-test (frame_kernel.hip
            // match_pairs_wide; tests/test_wide_pretest_bound_cpu.py) drops the clear misses, and the exact expression decides
            // what is left -- 1.6 blobs of 16 on the bench stream -- in ascending index, all lanes at once.  Without the float32
            // roundings the line is a double: the exact expression for all sixteen slots, straight line (a loop over the slots
            // under the count, one read and its wait per turn, measured 0.06 ms per 100 k frames SLOWER than the parent's walk).
            static_assert(ML % 2 == 0 && ML < 32, "two blobs per word, the slots as bits of one register");
            const float4* pw = (const float4*)pts;  // (bxy is 16-byte aligned, a camera's row is ML float2)
            uint32_t cand = (1u << Mi) - 1u;
            uint32_t hw = 0u;  // (the hits as one register: ML < 32)
            if constexpr (F32R) {
              // omax of the pre-test's bound: the largest coordinate any pair of the frame reads under its count (misc[MI_OMAX] is
              // filled later, with the per-blob table).  The frame's C ML slots are one word of two blobs per lane; the coordinates
              // compare as integers with the sign bit off (the order of the floats, NaN above +inf: a NaN under a count leaves the
              // bound at +inf, everything goes to the exact test), the wave's maximum by four row steps and the four rows' lanes.
              static_assert(CT * ML == 128, "the frame's slots: one word of two blobs per lane");
              uint32_t ob;
              {
                const float4 v = ((const float4*)bxy)[lane];
                const int n = cnt[lane / (ML / 2)], k0 = 2 * (lane % (ML / 2));
                const uint32_t ax = __float_as_uint(v.x) & 0x7FFFFFFFu, ay = __float_as_uint(v.y) & 0x7FFFFFFFu;
                const uint32_t az = __float_as_uint(v.z) & 0x7FFFFFFFu, aw = __float_as_uint(v.w) & 0x7FFFFFFFu;
                const uint32_t m0 = k0 < n ? (ax > ay ? ax : ay) : 0u, m1 = k0 + 1 < n ? (az > aw ? az : aw) : 0u;
                ob = m0 > m1 ? m0 : m1;
                auto up = [](uint32_t x, uint32_t y) { return x > y ? x : y; };
                ob = up(ob, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ob, 0xB1, 0xf, 0xf, true));   // quad_perm [1, 0, 3, 2]
                ob = up(ob, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ob, 0x4E, 0xf, 0xf, true));   // quad_perm [2, 3, 0, 1]
                ob = up(ob, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ob, 0x141, 0xf, 0xf, true));  // row_half_mirror
                ob = up(ob, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ob, 0x140, 0xf, 0xf, true));  // row_mirror
                const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)ob, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)ob, 16);
                const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)ob, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)ob, 48);
                ob = up(up(r0, r1), up(r2, r3));  // (wave-uniform: scalar from here)
                ob = ob < 0x7F800000u ? ob : 0x7F800000u;
              }
              const double om = (double)__uint_as_float(ob);
              const float a32 = (float)L.a, b32 = (float)L.b, c32 = (float)L.c;  // (exact: the line is float32)
              const float thr = f32_round_up(p.gate_px * L.den * (1.0 + 1e-12) + (2.5 * 0x1p-24) * (2.0 * om + fabs(L.c)) * (1.0 + 1e-6));
              // the camera's slots from the last to the first, a slot's verdict shifted in as the mask's lowest bit
              // (<= is false for NaN: an infinite or NaN slot or line passes only where thr is +inf, and then to the exact test)
              uint32_t pm = 0u;
#pragma unroll
              for (int h = ML / 2 - 1; h >= 0; h--) {
                const float4 v = pw[h];
                float t0 = fmaf(a32, v.x, fmaf(b32, v.y, c32)), t1 = fmaf(a32, v.z, fmaf(b32, v.w, c32));
                asm("" : "+v"(t0), "+v"(t1));  // (one scalar multiply-add each: as packed pairs they cost a move per operand)
                pm = pm + pm + (fabsf(t1) <= thr ? 1u : 0u);
                pm = pm + pm + (fabsf(t0) <= thr ? 1u : 0u);
              }
              cand &= pm;
              while (__ballot(cand != 0u)) {
                if (cand) {
                  const int k = __ffs((int)cand) - 1;
                  cand &= cand - 1u;
                  const double d = dist(k);
                  if (d < p.gate_px) {  // strict <, helpers.py:375,383
                    hw |= 1u << k;
                    if (d < bd0) {
                      bd0 = d;
                      bk0 = k;
                    }
                  }
                }
              }
            } else {
#pragma unroll
              for (int h = 0; h < ML / 2; h++) {
                const float4 v = pw[h];
                const double d0 = div_by(fabs(L.a * (double)v.x + L.b * (double)v.y + L.c), L.den, L.rden);  // helpers.py:373
                const double d1 = div_by(fabs(L.a * (double)v.z + L.b * (double)v.w + L.c), L.den, L.rden);
                // strict <, helpers.py:375,383; a slot at or beyond the count is no hit whatever it holds
                const bool h0 = d0 < p.gate_px && ((cand >> (2 * h)) & 1u), h1 = d1 < p.gate_px && ((cand >> (2 * h + 1)) & 1u);
                hw |= h0 ? 1u << (2 * h) : 0u;
                const bool b0 = h0 && d0 < bd0;
                bd0 = b0 ? d0 : bd0;
                bk0 = b0 ? 2 * h : bk0;
                hw |= h1 ? 2u << (2 * h) : 0u;
                const bool b1 = h1 && d1 < bd0;
                bd0 = b1 ? d1 : bd0;
                bk0 = b1 ? 2 * h + 1 : bk0;
              }
            }
            hm = hw;
          } else
#pragma unroll 4
          for (int k = 0; k < Mmax; k++)  // (unrolled by four; the emitted code runs the copies one after the other, each read waited for at once)
            if (k < Mi && dist(k) < p.gate_px) hm |= 1ull << k;  // strict <, helpers.py:375,383
          uint8_t* nhp = stage == 0 ? nh : nh_s;
          uint8_t* hl = (stage == 0 ? hits : hits_s) + ((size_t)r * C + i) * M;
          if (have) nhp[(size_t)r * C + i] = (uint8_t)__popcll(hm);
          // order by (distance, blob index): a stable order where NumPy's default argsort is not (helpers.py:384;
          // documented deviation); the closest hit's coordinates claim every blob that has them (helpers.py:391)
          unsigned long long rem = hm, claim = 0ull;
          int pos = 0;
          float2 p0 = make_float2(0.f, 0.f);
          if constexpr (ROWS) {
            // position 0 is the walk's minimum; a list of one claims itself (a hit's coordinates are finite: equal to themselves);
            // below, the last hit left of any list is placed without a distance -- no distance is computed twice for lists of
            // up to two, the usual ones
            if (hm) {
              hl[0] = (uint8_t)gbyte(i, (uint32_t)bk0);
              claim = hm;
              if (hm & (hm - 1ull)) {
                claim = 0ull;
                p0 = pts[bk0];
                for (unsigned long long t = hm; t; t &= t - 1) {
                  const int k = __ffsll((long long)t) - 1;
                  const float2 q = pts[k];
                  if (q.x == p0.x && q.y == p0.y) claim |= 1ull << k;
                }
              }
              rem = hm & ~(1ull << bk0);
              pos = 1;
            }
          }
          while (__ballot(rem != 0ull)) {
            if (rem) {
              double bd = __builtin_huge_val();
              int bk = 0;
              if (ROWS && !(rem & (rem - 1ull))) {
                bk = __ffsll((long long)rem) - 1;
              } else
              for (unsigned long long t = rem; t; t &= t - 1) {  // ascending index, strict <: ties keep the smaller index
                const int k = __ffsll((long long)t) - 1;
                const double d = dist(k);
                if (d < bd) {
                  bd = d;
                  bk = k;
                }
              }
              hl[pos] = (uint8_t)gbyte(i, (uint32_t)bk);
              if (!ROWS && pos == 0) {
                p0 = pts[bk];
                for (unsigned long long t = hm; t; t &= t - 1) {
                  const int k = __ffsll((long long)t) - 1;
                  const float2 q = pts[k];
                  if (q.x == p0.x && q.y == p0.y) claim |= 1ull << k;
                }
              }
              rem &= ~(1ull << bk);
              pos++;
            }
          }
          if (stage == 0) {
            if (claim) atomicOr(&claimw[i], claim);
          } else if (have) {
            pclaim[(size_t)r * C + i] = claim;
          }
        }
      }
    }
    // Speculative lines (only for frames that take the old chain): the epipolar lines of the blobs that might become roots
    // depend on nothing, so all waves compute them off the chain's critical path.  Table = the search's dead arrays: line
    // (j, k) -> i at sp_base(j) + k (C-1-j) + (i-j-1), float32 a, b, c (F32R: that is what they are, helpers.py:364) + den.
    const int NL = M * ((C - 1) * (C - 2) / 2);
    const bool spec = F32R && (size_t)NL * 20 + 8 <= scr_bytes;
    double* sp_den = (double*)scr;
    float* sp_abc = (float*)(sp_den + NL);
    auto sp_base = [&](int j) { return M * ((j - 1) * (C - 1) - (j - 1) * j / 2); };  // lines of cameras 1 .. j-1
    // ... of the blobs the camera-0 roots have NOT claimed only (a claimed blob never becomes a root): one lane per
    // (unclaimed blob, later camera) pair, ~40 lines per frame.
    if (spec && !pre) {  // (behind stage 0's barrier: the claim words are complete)
      int tot = 0;
      for (int j = 1; j <= C - 2; j++) {
        const int n = cnt[j];
        const unsigned long long U = ~claimw[j] & (n >= 64 ? ~0ull : ((1ull << n) - 1ull));
        tot += __popcll(U) * (C - 1 - j);
      }
      for (int l = tid; l < tot; l += T) {
        int j = 1, acc = 0, span = C - 2;
        unsigned long long U = 0ull;
        for (; j <= C - 2; j++) {
          const int n = cnt[j];
          U = ~claimw[j] & (n >= 64 ? ~0ull : ((1ull << n) - 1ull));
          span = C - 1 - j;
          const int nj = __popcll(U) * span;
          if (l < acc + nj) break;
          acc += nj;
        }
        uint32_t ord, off;
        divmod_tiny((uint32_t)(l - acc), (uint32_t)span, ord, off);  // (< 64 x 15, span <= 14)
        for (uint32_t t = 0; t < ord; t++) U &= U - 1;
        const int k = __ffsll((long long)U) - 1, i = j + 1 + (int)off;
        const int ll = sp_base(j) + k * span + (int)off;
        const Line L = epiline_of(j, k, i);
        sp_den[ll] = L.den;
        sp_abc[3 * ll + 0] = (float)L.a;
        sp_abc[3 * ll + 1] = (float)L.b;
        sp_abc[3 * ll + 2] = (float)L.c;
      }
    }
    __syncthreads();
    pc_mark<PC_PAIRS1>();
    fresh_tid();
    if (wave == 0) bb_prio<kPrioSerial>();
    if (wave == 0 && pre) {
      // B1, pre-matched: lane p <-> provisional root p = the p-th unclaimed blob of cameras 1 .. C-1 in (camera, blob) order.
      // A provisional root is real when no root created at an earlier camera claims its blob (helpers.py:391,402-406).
      int jp = 0, kp = 0;
      if constexpr (PLIST) {
        if (lane < n_prov) {  // (the list: every wave wrote it before stage 1, two barriers ago)
          const int row = plist[lane];
          jp = row / ML;
          kp = row & (ML - 1);
        }
      } else
      if (lane < n_prov) {
        int acc = 0;
        unsigned long long U = 0ull;
        for (jp = 1; jp < C; jp++) {
          U = U_of(jp);
          const int np = __popcll(U);
          if (lane < acc + np) break;
          acc += np;
        }
        for (int t = 0; t < lane - acc; t++) U &= U - 1;
        kp = __ffsll((long long)U) - 1;
      }
      // Camera by camera: the provisional roots of camera i look their blob up in the camera's claim word; the real ones add
      // their own claims to the words of the cameras after them (the claim words end up as the reference's "claimed" sets).
      // One LDS read and a handful of atomics per camera -- a wave-wide OR by shuffles was 12 dependent cross-lane operations per camera.
      bool real = false;
      for (int i = 1; i < C; i++) {
        wave_lds_sync();
        if (lane < n_prov && jp == i) {
          real = !((claimw[i] >> kp) & 1ull);
          if (real)
            for (int c = i + 1; c < C; c++) {
              const unsigned long long m = pclaim[(size_t)lane * C + c];
              if (m) atomicOr(&claimw[c], m);
            }
        }
      }
      const unsigned long long rm = __ballot(real);
      const int rank = __popcll(rm & ((1ull << lane) - 1ull));
      int n_roots = n0 + __popcll(rm);
      if (real && n0 + rank < R) {
        root_cam[n0 + rank] = (uint8_t)jp;
        root_blob[n0 + rank] = (uint8_t)kp;
        bnl[rank] = (uint8_t)lane;  // (bnl is dead until phase C: the staging row of the rank-th new root)
      }
      if (lane == 0) {
        if (n_roots > R) {
          misc[MI_STATUS] |= MOCAP_ST_ROOT_OVERFLOW_;
          n_roots = R;
        }
        misc[MI_NROOTS] = n_roots;
      }
    } else if (wave == 0) {
      // B1: the chain over the cameras -- only the roots created on the way take part (camera-0 roots are done).
      // State in registers: lane l <-> camera l (blob count, blobs claimed so far), lane l <-> the l-th new root.
      const int cntL = lane < C ? cnt[lane] : 0;
      const unsigned long long clmL = lane < C ? claimw[lane] : 0ull;  // the camera-0 roots' claims (B0 is complete)
      int nr_cam = 0, nr_blob = 0;
      int n_roots = n0;
      bool over = false;
      for (int i = 1; i < C; i++) {
        const int Mi = __builtin_amdgcn_readlane(cntL, i);
        unsigned long long claimed = ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)(clmL >> 32), i) << 32) |
                                     (unsigned int)__builtin_amdgcn_readlane((int)clmL, i);
        const int n_new = n_roots - n0;
        for (int base = 0; base < n_new; base += 64) {
          const int l = base + lane;
          const bool have = l < n_new;  // created at an earlier camera
          int j = nr_cam, k = nr_blob;
          if (base) {                   // (beyond the 64 kept in registers: from the root arrays this wave wrote)
            wave_lds_sync();
            j = have ? root_cam[n0 + l] : 0;
            k = have ? root_blob[n0 + l] : 0;
          }
          Line L = {0, 0, 0, 1, 1};
          if (have) {
            if (spec) {
              const int ll = sp_base(j) + k * (C - 1 - j) + (i - j - 1);
              L.a = (double)sp_abc[3 * ll + 0];
              L.b = (double)sp_abc[3 * ll + 1];
              L.c = (double)sp_abc[3 * ll + 2];
              L.den = sp_den[ll];
              L.rden = recip_refined(L.den);
            } else {
              L = epiline_of(j, k, i);
            }
          }
          claimed |= match_pairs<true>(L, n0 + l, i, (n_new - base < 64) ? n_new - base : 64, gs_shift, i, Mi);
        }
        // unclaimed blobs become new roots, in blob order (helpers.py:402-406)
        const bool flag = lane < Mi && !((claimed >> lane) & 1ull);
        const unsigned long long mask = __ballot(flag);
        const int pos = __popcll(mask & ((1ull << lane) - 1ull));
        if (flag) {
          const int rr = n_roots + pos;
          if (rr < R) {
            root_cam[rr] = (uint8_t)i;
            root_blob[rr] = (uint8_t)lane;
          }
        }
        int slot = n_new;
        for (unsigned long long mm = mask; mm; slot++) {  // wave-uniform: the new roots' registers
          const int jb = __ffsll((long long)mm) - 1;
          mm &= mm - 1;
          if (lane == slot) {
            nr_cam = i;
            nr_blob = jb;
          }
        }
        n_roots += __popcll(mask);
        if (n_roots > R) {
          over = true;
          n_roots = R;
        }
      }
      if (lane == 0) {
        if (over) misc[MI_STATUS] |= MOCAP_ST_ROOT_OVERFLOW_;
        misc[MI_NROOTS] = n_roots;
      }
    } else {
      // meanwhile: DLT contribution of every blob, once per frame (a candidate group then ADDS ten doubles per view),
      // and the largest coordinate (float32 allowance of the bounds)
      float om = 0.0f;
      for (int i = tid - 64; i < C * M; i += T - 64) {
        const int c = i / M, k = i - c * M;
        if (k < cnt[c]) {
          const float2 v = bxy[i];
          om = fmaxf(om, fmaxf(fabsf(v.x), fabsf(v.y)));
          double Bc[10];
          dlt_contribution(Bc, cv.pq(PERK ? 12 * (c * C + c) : 12 * c), (double)v.x, (double)v.y);
#pragma unroll
          for (int e = 0; e < 10; e++) bt[(size_t)i * 10 + e] = Bc[e];
        }
      }
      if (om > 0.0f) atomicMax(&misc[MI_OMAX], __float_as_int(om));
      if (tid == 64) {
        const int it = q_add(&p.q.counters[QC_NEXT_FRAME], 1);
        misc[MI_NEXT] = it < frame_count(p) ? it : -1;
      }
    }
    bb_prio<kPrioPhase>();
    __syncthreads();
    pc_mark<PC_B1_TABLE>();
    if (pre) {
      // the real provisional roots' rows leave the staging area for their final place: one lane per (new root, camera)
      const int n_new = misc[MI_NROOTS] - n0;
      for (int idx = tid; idx < n_new * C; idx += T) {
        const int q = idx / C, c = idx - q * C;
        const int r = n0 + q, ps = bnl[q];
        if (c > (int)root_cam[r]) {
          const int n = nh_s[(size_t)ps * C + c];
          nh[(size_t)r * C + c] = (uint8_t)n;
          const uint8_t* src = hits_s + ((size_t)ps * C + c) * M;
          uint8_t* dst = hits + ((size_t)r * C + c) * M;
          for (int t = 0; t < n; t++) dst[t] = src[t];
        }
      }
      __syncthreads();  // (the staging rows are the search's arrays: phase C initialises them next)
      pc_mark<PC_ROW_COPY>();
    }

    // C: candidate counts per root
    fresh_tid();
    const int nroots = misc[MI_NROOTS];
    for (int r = tid; r < nroots; r += T) {
      if constexpr (ROWS) {
        // the same per root from registers: the nh row as one word, the first hit of every camera read unconditionally (independent
        // reads; a single-hit camera's is used), the act row built in a register and stored once, the block size from the digits'
        // counts kept beside it -- no load behind a store, no a[k] -> nh[...] chain
        const uint32_t rc = root_cam[r], rb = root_blob[r];
        unsigned long long nw = row_word64(nh, r);
        const uint8_t* hr = hits + (size_t)r * (CT * ML);
        uint32_t h1[CT];
#pragma unroll
        for (int c = 1; c < CT; c++) h1[c] = hr[c * ML];
        // cameras at or below the root's own: nothing writes their bytes for this root (stage 0 writes cameras >= 1 of camera-0
        // roots, the row copy c > root_cam) -- whatever an earlier frame's root left in the slot is masked out
        nw &= (~0ull << (8u * rc)) << 8;
        Pk pkb;
        pkb.clear();
        pkb.set((int)rc, gbyte((int)rc, rb));
        // the digits, one byte each: camera | (hit count - 1) << 3 (c <= 7, counts <= ML = 16), pushed from the last camera down
        // so that digit 0, the lowest multi-hit camera, ends up in the low byte -- shifts by a constant only
        static_assert(CT <= 8 && ML <= 16, "a digit's byte: three bits of camera, four of hit count - 1");
        unsigned long long ew = 0ull;
        uint32_t total = 1, views = 1, na = 0, sm = 1u << rc;  // (total: seven counts <= 16 -> < 2^32)
#pragma unroll
        for (int c = CT - 1; c >= 1; c--) {
          const uint32_t n = byte_of(nw, (uint32_t)c);
          if (n > 1) {
            ew = (ew << 8) | (unsigned long long)((n << 3) + (uint32_t)(c - 8));
            na++;
          }
          if (n == 1) pkb.set(c, h1[c]);
          if (n) {
            sm |= 1u << c;
            views++;
            total *= n;
          }
        }
        const unsigned long long aw = ew & 0x0707070707070707ull;                                   // the act row: the digits' cameras
        const unsigned long long dn = ((ew >> 3) & 0x0F0F0F0F0F0F0F0Full) + 0x0101010101010101ull;  // the digits' hit counts (1 beyond na: not read)
        // (the loop's rule: over as soon as a prefix product exceeds G_cap -- counts are >= 1, the products monotone: the full one decides)
        const bool over = (unsigned long long)total > (unsigned long long)p.G_cap;
        if (over) atomicOr(&misc[MI_STATUS], MOCAP_ST_CAND_OVERFLOW_);
        ((unsigned long long*)act)[r] = aw;
        nact[r] = (uint8_t)na;
        bv[r] = (uint8_t)views;
        pkbase[r] = pkb.w[0];
        if (PERK) seen[r] = (uint16_t)sm;
        rbound[r] = kInfBits;
        const uint32_t g = (views > 1 && !over) ? total : 0u;
        gcnt[r] = g;
        uint32_t pl = 1, nb = over ? 1u : total;  // (the multi-hit counts' product = total: single hits contribute 1)
        uint32_t nl = 0;
        while (nl < na && (pl < (uint32_t)p.bb_pl_min || (pl < (uint32_t)p.bb_pl && nb > (uint32_t)p.bb_nb_max))) {
          const uint32_t n = byte_of(dn, nl++);
          uint32_t dummy;
          pl *= n;
          divmod_small(nb, n, nb, dummy);  // (exact: nb < 2^24 is a multiple of n)
        }
        bpl[r] = (uint16_t)pl;
        bnl[r] = (uint8_t)nl;
        bnb[r] = g ? nb : 0u;
        seedkey[r] = 0ull;
        seedgh[r] = 0xFFFFFFFFu;
        continue;
      }
      const int rc = root_cam[r];
      unsigned long long total = 1;
      int views = 1, na = 0;
      bool over = false;
      // what every block of the root has in common (block_pk): the root's own blob and the single-hit cameras' blobs
      Pk pkb;
      pkb.clear();
      pkb.set(rc, gbyte(rc, root_blob[r]));
      uint32_t sm = 1u << rc;
      for (int c = rc + 1; c < C; c++) {
        const unsigned n = nh[(size_t)r * C + c];
        if (n > 1) act[(size_t)r * C + na++] = (uint8_t)c;  // multi-hit cameras = the digits of the candidate index
        if (n == 1) pkb.set(c, hits[((size_t)r * C + c) * M]);
        if (n) {
          sm |= 1u << c;
          views++;
          total *= n;
          if (total > (unsigned long long)p.G_cap) {
            over = true;
            total = 1;
          }
        }
      }
      if (over) atomicOr(&misc[MI_STATUS], MOCAP_ST_CAND_OVERFLOW_);
      nact[r] = (uint8_t)na;
      bv[r] = (uint8_t)views;
#pragma unroll
      for (int k = 0; k < CW; k++) pkbase[(size_t)r * CW + k] = pkb.w[k];
      if (PERK) seen[r] = (uint16_t)sm;
      rbound[r] = kInfBits;
      const uint32_t g = (views > 1 && !over) ? (uint32_t)total : 0u;  // helpers.py:413-414 drops 1-view roots
      gcnt[r] = g;
      // the search's blocks of this root (phase D): the nl fastest digits stay open (pl candidates per block), one block per
      // value of the others.  The size is the root's own: digits open until a block holds bb_pl_min candidates, and further -- up
      // to bb_pl -- while more than bb_nb_max blocks would be left.  A root with few candidates gets small blocks (its seed block,
      // evaluated against no bound at all, is most of what it costs), one with many keeps the number of bounds in check.
      // Here rather than at the start of the search: the same lanes, no extra barrier pair.
      {
        const uint8_t* a = act + (size_t)r * C;
        uint32_t pl = 1, nb = 1;
        int nl = 0;
        for (int k = 0; k < na; k++) nb *= nh[(size_t)r * C + a[k]];  // (= total; 1 for a root over G_cap, which has no blocks)
        if (over) nb = 1;
        while (nl < na && (pl < (uint32_t)p.bb_pl_min || (pl < (uint32_t)p.bb_pl && nb > (uint32_t)p.bb_nb_max))) {
          const uint32_t n = nh[(size_t)r * C + a[nl++]];
          uint32_t dummy;
          pl *= n;
          divmod_small(nb, n, nb, dummy);  // (exact: nb < 2^24 is a multiple of n)
        }
        bpl[r] = (uint16_t)pl;
        bnl[r] = (uint8_t)nl;
        bnb[r] = g ? nb : 0u;
        seedkey[r] = 0ull;  // (the speculative lines that lived here are dead: the chain is behind the barrier above)
        seedgh[r] = 0xFFFFFFFFu;
      }
    }
    for (int s = tid; s < W * RS; s += T) {
      slot_key[s] = ~0ull;
      slot_g[s] = 0xFFFFFFFFu;
    }
    if (tid == 0) misc[MI_BBCTR] = misc[MI_BBCTR2] = 0;
    __syncthreads();
    if (wave == 0) bb_prio<kPrioSerial>();
    if (wave == 0) {  // candidate offsets, block offsets and output slots: scans over the roots, 64 at a time (sums stay below 2^32: 255 x 2^24)
      uint32_t carry = 0, bcarry = 0;
      int slots = 0;
      for (int base = 0; base < nroots; base += 64) {
        const int r = base + lane;
        const uint32_t g = r < nroots ? gcnt[r] : 0u;
        const uint32_t nb = r < nroots ? bnb[r] : 0u;
        const uint32_t incl = wave_inclusive_scan(g, lane);
        const uint32_t bincl = wave_inclusive_scan(nb, lane);
        const unsigned long long nz = __ballot(g != 0u);
        if (r < nroots) {
          goff[r] = carry + incl - g;
          boff[r] = bcarry + bincl - nb;
          outslot[r] = g ? slots + __popcll(nz & ((1ull << lane) - 1ull)) : -1;
        }
        carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        bcarry += (uint32_t)__builtin_amdgcn_readlane((int)bincl, 63);
        slots += __popcll(nz);
      }
      if (lane == 0) {
        goff[nroots] = carry;
        boff[nroots] = bcarry;
        misc[MI_NOUT] = slots;
        misc[MI_G] = misc[MI_STATUS] ? 0 : (int32_t)carry;
      }
    }
    bb_prio<kPrioPhase>();
    __syncthreads();
    pc_mark<PC_PHASE_C>();
  }

  // ---------------------------------------------------------------- phase D
  // DLT matrix of candidate `rem` of root r with the first `skip` multi-hit cameras left open (skip = 0: the whole
  // group, rem = candidate index; skip = bnl[r]: the block's partial group, rem = block index).  Returns the views.
  // B += the DLT contribution of blob k of camera c, the camera at position j among the group's seen cameras
  __device__ __forceinline__ void add_view(double (&B)[10], int c, uint32_t k, int j) const {  // k: the group's byte
    if (PERK && j != c) {
      const float2 w = bxy[grow(c, k)];
      double Bc[10];
      dlt_contribution(Bc, cv.base + 12 * ((size_t)j * cn() + c), (double)w.x, (double)w.y);  // (per-lane position: vector loads, L1/L2-resident table)
#pragma unroll
      for (int e = 0; e < 10; e++) B[e] = B[e] + Bc[e];
    } else {
      const double* t = bt + grow(c, k) * 10;
#pragma unroll
      for (int e = 0; e < 10; e++) B[e] = B[e] + t[e];
    }
  }

  template <bool WITH_B>
  __device__ __forceinline__ int group_matrix(int r, uint32_t rem, int skip, double (&B)[10], Pk& pk) const {
    const int C = cn();
    const int rc = root_cam[r];
    const uint8_t* nhr = nh + (size_t)r * C;
    const uint8_t* hr = hits + (size_t)r * C * M;
    pk.clear();
    int v = 0, ka = 0;
    int j = 0;  // PERK: position of camera c among the root's seen cameras -- the open ones of a partial group count
    if (WITH_B) {
#pragma unroll
      for (int e = 0; e < 10; e++) B[e] = 0.0;
    }
    for (int c = 0; c < C; c++) {
      uint32_t k = kNone;
      bool seen = false;
      if (c == rc) {
        k = gbyte(c, root_blob[r]);
        seen = true;
      } else if (c > rc) {
        const uint32_t n = nhr[c];
        seen = n != 0;
        if (n == 1) {
          k = hr[(size_t)c * M];
        } else if (n > 1) {
          if (ka >= skip) {
            uint32_t qd, dgt;
            if (rem < 8192u) divmod_tiny(rem, n, qd, dgt); else  // (the usual case for every lane of the wave: one path runs)
            divmod_small(rem, n, qd, dgt);
            rem = qd;
            k = hr[(size_t)c * M + dgt];
          }
          ka++;
        }
      }
      if (k != kNone) {
        if (WITH_B) add_view(B, c, k, j);
        v++;
        pk.set(c, k);
      }
      if (PERK) j += seen ? 1 : 0;
    }
    return v;
  }

  // Blob indices of block gh of root r: what the root's blocks share (pkbase: the root's blob, the single-hit cameras) plus the
  // block's own fixed digits -- the multi-hit cameras act[bnl[r] .. nact[r]-1], typically one to three; the open digits' and the
  // absent cameras' bytes stay kNone.  (group_matrix walks all cameras for the same bytes; it remains the self-check build's decoder.)
  __device__ __forceinline__ void block_pk(int r, uint32_t gh, Pk& pk) const {
    const int C = cn();
#pragma unroll
    for (int k = 0; k < CW; k++) pk.w[k] = pkbase[(size_t)r * CW + k];
    if constexpr (ROWS) {
      // the root's digits and hit counts as two words, read next to the sizes: a digit's camera and count are shifts, only its
      // hits byte is a dependent read
      const unsigned long long aw = row_word64(act, r), nw = row_word64(nh, r);
      const int na = nact[r];
      const uint8_t* hr = hits + (size_t)r * (CT * ML);
      uint32_t rem = gh;
      for (int k = bnl[r]; k < na; k++) {
        const uint32_t c = byte_of(aw, (uint32_t)k), n = byte_of(nw, c);
        uint32_t qd, dgt;
        if (rem < 8192u) divmod_tiny(rem, n, qd, dgt); else
        divmod_small(rem, n, qd, dgt);
        rem = qd;
        pk.set((int)c, hr[c * (uint32_t)ML + dgt]);
      }
      return;
    }
    const uint8_t* a = act + (size_t)r * C;
    const int na = nact[r];
    uint32_t rem = gh;
    for (int k = bnl[r]; k < na; k++) {
      const int c = a[k];
      const uint32_t n = nh[(size_t)r * C + c];
      uint32_t qd, dgt;
      if (rem < 8192u) divmod_tiny(rem, n, qd, dgt); else  // (the usual case for every lane of the wave: one path runs)
      divmod_small(rem, n, qd, dgt);
      rem = qd;
      pk.set(c, hits[((size_t)r * C + c) * M + dgt]);
    }
  }
  // ... and the DLT matrix of the block's partial group: the table rows of its cameras in ascending order, branch-free -- a camera
  // that is open or absent adds the record of zeros, as in fetch_candidate (same bits as skipping it).  Per-camera K: a view's
  // position is the number of SEEN cameras before it, the open ones included (the root's `seen` mask), add_view's rule.
  // Returns the views of the partial group.
  __device__ __forceinline__ int block_matrix(int r, uint32_t gh, Pk& pk, double (&B)[10]) const {
    const int C = cn();
    block_pk(r, gh, pk);
#pragma unroll
    for (int ee = 0; ee < 10; ee++) B[ee] = 0.0;
    if constexpr (PERK) {
      const uint32_t sm = seen[r];
#pragma unroll CT > 0 ? CT : 1
      for (int c = 0; c < C; c++) {
        const uint32_t k = pk.get(c);
        if (k != kNone) add_view(B, c, k, __popc(sm & ((1u << c) - 1u)));
      }
    } else {
#pragma unroll CT > 0 ? CT : 1
      for (int c = 0; c < C; c++) {
        const uint32_t k = pk.get(c);
        const double* t = bt + (size_t)(ROWS ? k : k != 0xFFu ? (uint32_t)c * (uint32_t)M + k : (uint32_t)C * (uint32_t)M) * 10;
#pragma unroll
        for (int ee = 0; ee < 10; ee++) B[ee] = B[ee] + t[ee];
      }
    }
    return (int)bv[r] - (int)bnl[r];
  }

  // Record r of the queue and candidate i of the expanded list -> the candidate's root, index, blob indices and DLT matrix
  // (cameras in ascending order: the one canonical rounding of B; a camera that is not in the group adds the table's record
  // of zeros: x + (+0.0) = x for every x the sum can hold -- it starts at +0.0, so it is never -0.0 -- the same bits
  // without a save-exec / branch / restore around every camera).  Returns the views (the root's: every candidate of a root
  // has the same cameras).
  __device__ __forceinline__ int fetch_candidate(uint32_t lo, uint32_t i, int& r, uint32_t& gl, Pk& pk, double (&B)[10]) const {
    const int C = cn();
    const BRec rec = recs[lo];
    r = (int)(rec.rs & 0xFFu);
#pragma unroll
    for (int k = 0; k < CW; k++) pk.w[k] = rpk[(size_t)lo * CW + k];
    if (rec.rs >> 31) {
      gl = rec.gh;  // a single candidate: its blob indices are complete
    } else {
      uint32_t rem = i - (rec.rs >> 8);
      gl = rec.gh * (uint32_t)bpl[r] + rem;
      const uint8_t* a = act + (size_t)r * C;
      const int nl = bnl[r];
      if constexpr (ROWS) {
        const unsigned long long aw = row_word64(act, r), nw = row_word64(nh, r);  // (independent of each other and of bpl / bnl)
        const uint8_t* hr = hits + (size_t)r * (CT * ML);
        for (int k = 0; k < nl; k++) {
          const uint32_t c = byte_of(aw, (uint32_t)k);
          uint32_t qd, dgt;
          divmod_tiny(rem, byte_of(nw, c), qd, dgt);
          rem = qd;
          pk.set((int)c, hr[c * (uint32_t)ML + dgt]);
        }
      } else
      for (int k = 0; k < nl; k++) {  // the block's open digits (rem < pl < 2^13, hit counts <= 64: divmod_tiny is exact)
        const int c = a[k];
        uint32_t qd, dgt;
        divmod_tiny(rem, nh[(size_t)r * C + c], qd, dgt);
        rem = qd;
        pk.set(c, hits[((size_t)r * C + c) * M + dgt]);
      }
    }
#pragma unroll
    for (int ee = 0; ee < 10; ee++) B[ee] = 0.0;
    if constexpr (PERK) {
      int j = 0;  // (the group is complete: its cameras are the root's seen cameras)
#pragma unroll CT > 0 ? CT : 1
      for (int c = 0; c < C; c++) {
        const uint32_t k = pk.get(c);
        if (k != kNone) add_view(B, c, k, j++);
      }
    } else {
#pragma unroll CT > 0 ? CT : 1
      for (int c = 0; c < C; c++) {
        const uint32_t k = pk.get(c);
        const double* t = bt + (size_t)(ROWS ? k : k != 0xFFu ? (uint32_t)c * (uint32_t)M + k : (uint32_t)C * (uint32_t)M) * 10;
#pragma unroll
        for (int ee = 0; ee < 10; ee++) B[ee] = B[ee] + t[ee];
      }
    }
    return bv[r];
  }

  __device__ void search(bool bound_tests) {
    fresh_tid();
    const int C = cn();
    (void)C;
    // Barriers: the rounds of the search exchange LDS state only, so its inner barriers are block_sync_lds_only() -- a round
    // does not wait for the L2 acknowledgement of its winner-record stores (phase E reads them behind wait_own_stores() and the
    // search's LAST barrier, which stays a full one).
    // The wait below: the compiler cannot tell the prefetch's LDS target from any other LDS address and waits for vmcnt(0)
    // before the first LDS access behind a global_load_lds on every path that has not waited yet -- with the frame's prefetch
    // pending that was before each view's blob read and each delivery atomic of the evaluation (11 waits per pass, each also
    // a wait for the pass's record stores).  One wait it can see, here, where the first LDS read would have waited anyway.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) alone (gfx9 encoding: expcnt 7, lgkmcnt 15)
    const int nroots = misc[MI_NROOTS];
    // queued records | their candidates << 10.  Two words that take turns: a flush moves on to the other one (zero since the
    // flush before), and lane 0 zeroes the one just used behind the round's barrier -- nobody touches it until the next
    // flush has passed its own barrier: one barrier per evaluation round instead of two
    int32_t* ctr = &misc[MI_BBCTR];
    int32_t* ctr_other = &misc[MI_BBCTR2];
    const double inf = __builtin_huge_val();
    EigCut ec;
    {
      const double om = (double)__int_as_float(misc[MI_OMAX]);
      ec.p3max2 = p.p3max2;
      ec.o2slack = (1100.0 * 0x1p-46) * (om * om);
    }
    const double c0[3] = {p.bb_c0[0], p.bb_c0[1], p.bb_c0[2]};  // origin of the frame the block bounds are taken in
    // (blocks per root, their offsets, the result slots and the queue counters were set up with the candidate counts: match(), phase C)
    const uint32_t nblocks = boff[nroots];
    // root of block b0 + tid (consecutive blocks per wave): last root whose first block is <= b
    auto root_of_block = [&](uint32_t b_first_of_wave, uint32_t b) {
      return coop_last_le([&](int r) { return boff[r]; }, nroots, b_first_of_wave, b, lane);
    };
    auto push_block = [&](int r, uint32_t gh, const Pk& pk) {
      const uint32_t old = (uint32_t)atomicAdd(ctr, (int32_t)(((uint32_t)bpl[r] << 10) | 1u));
      const uint32_t slot = old & 0x3FFu;
      BRec rec;
      rec.gh = gh;
      rec.rs = (uint32_t)r | ((old >> 10) << 8);
      recs[slot] = rec;
#pragma unroll
      for (int k = 0; k < CW; k++) rpk[(size_t)slot * CW + k] = pk.w[k];
    };
    auto rec_start = [&](int k) { return (recs[k].rs & 0x7FFFFFFFu) >> 8; };
    // EigCut's first test of a (partial) group of root r against the best error of the root so far
    // (root_y: the root's side of the test -- p3max2c times the limit its best error so far sets, with the allowances)
    auto root_y = [&](int r) {
      const int vf = bv[r];
      const double bound = __longlong_as_double((long long)rbound[r]);
      const double limit = bound * (double)(2 * vf) * (1.0 + 0x1p-40);
      const double limit_adj = fma(1.002, limit, (double)(2 * vf) * ec.o2slack);
      return p.p3max2c * limit_adj;
    };
    auto dropped = [&](int r, double s1, double tr) { return s1 * fma(2e-12, tr, root_y(r)) < 1.0; };
    if (bound_tests) {
      bb_prio<kPrioSeed>();
      // ---- 1. seeds: s1 of every block (cached for the tests); per root the block with the largest s1 (smallest
      // bound) almost always holds the winner
      // (a frame of at most T blocks -- the usual one -- takes one trip through this loop: the lane that turns out to hold its
      // root's seed block queues it itself afterwards, with the blob indices it has, instead of one lane per root decoding them again)
      int my_r = -1;
      uint32_t my_gh = 0;
      unsigned long long my_key = 0ull;
      Pk my_pk;
      my_pk.clear();
      for (uint32_t s0 = 0; s0 < nblocks; s0 += T) {
        const uint32_t b = s0 + (uint32_t)tid;
        if (s0 + (uint32_t)(wave * 64) >= nblocks) continue;  // wave-uniform
        const int r = root_of_block(s0 + (uint32_t)(wave * 64), b < nblocks ? b : nblocks - 1);
        if (b < nblocks) {
          const uint32_t gh = b - boff[r];
          double B[10], tr = 0.0;
          Pk pk;
          const int v = block_matrix(r, gh, pk, B);
          double s1d = __builtin_huge_val();  // a one-view partial group carries no information: never dropped, any seed
          float s1 = 0.0f;
          if (v >= 2) {
            s1d = eigcut_s1_shifted(B, c0, tr);
            s1 = (float)fmin(s1d, 3e38);
          }
          if (b < (uint32_t)ncache) bcache[b] = v >= 2 ? bb_fold_bound(s1d, tr) : bb_fold_inf();
          my_key = ((unsigned long long)__float_as_uint(s1) << 32) | (unsigned long long)(0xFFFFFFFFu - gh);
          my_r = r;
          my_gh = gh;
          my_pk = pk;
          atomicMax(&seedkey[r], my_key);
        }
      }
      block_sync_lds_only();
      pc_mark<PC_SEED_PASS>();
      if (nblocks <= (uint32_t)T) {
        if (my_r >= 0 && seedkey[my_r] == my_key) {  // (keys are unique inside a root: exactly one lane per root with blocks)
          seedgh[my_r] = my_gh;
          push_block(my_r, my_gh, my_pk);
        }
      } else
      for (int r = tid; r < nroots; r += T) {
        if (bnb[r]) {
          const uint32_t gh = 0xFFFFFFFFu - (uint32_t)seedkey[r];
          seedgh[r] = gh;
          seedkey[r] = 0ull;
          Pk pk;
          block_pk(r, gh, pk);
          push_block(r, gh, pk);
        }
      }
      bb_prio<kPrioEval>();
      block_sync_lds_only();
      pc_mark<PC_SEED_PUSH>();
    }
    // ---- 2. the queued records' candidates (spread over all lanes, whatever root they belong to), then the next
    // blocks' tests, until nothing is left
    uint32_t b0 = 0;
    fresh_tid();
    while (true) {
      const uint32_t cv_ = (uint32_t)*ctr;
      const uint32_t ns = cv_ & 0x3FFu, ne = cv_ >> 10;
      const bool blocks_left = b0 < nblocks;
      const bool full = ns > (uint32_t)(kBBRecs - T);
      if (ns && (full || !blocks_left || ne >= (uint32_t)p.bb_flush)) {
        for (uint32_t i0 = 0; i0 < ne; i0 += T) {
          const uint32_t i = i0 + (uint32_t)tid;
          const bool have = i < ne;
          double e = inf, X[3] = {0, 0, 0};
          int r = 0;
          uint32_t gl = 0;
          // the record that candidate i of the expanded list belongs to: last one starting at or before i
          uint32_t lo = 0;
          if (i0 + (uint32_t)(wave * 64) < ne)  // wave-uniform
            lo = (uint32_t)coop_last_le(rec_start, (int)ns, i0 + (uint32_t)(wave * 64), have ? i : ne - 1, lane);
          Pk pk;  // the candidate's blob bytes: they go into the winner's record with the point
          pk.clear();
          if (have) {
            double B[10];
            const int v = fetch_candidate(lo, i, r, gl, pk, B);
            if constexpr (ROWS) {
              // (the table sum and the views below take the same eight bytes: extracted once, they would stay in eight registers
              // across the whole solve -- the views extract theirs again from the two words)
#pragma unroll
              for (int k = 0; k < CW; k++) asm volatile("" : "+v"(pk.w[k]));
            }
            auto obs_p = [&](int c, double& x, double& y) -> bool {
              const uint32_t k = pk.get(c);
              if (k == kNone) return false;
              const float2 w = bxy[grow(c, k)];
              x = (double)w.x;
              y = (double)w.y;
              return true;
            };
            const double bound = __longlong_as_double((long long)rbound[r]);
            solve_and_score<!PERK, true, F32R, false, 1, true>(cv, B, v, obs_p, X, e, bound * (double)(2 * v) * (1.0 + 0x1p-40), ec);
#ifdef MOCAP_DEBUG_EIGCHECK  // self-check build: a candidate whose evaluation was cut short must not beat the bound it was cut against
            if (!(e < inf)) {
              double B2[10], X2[3], e2;
#pragma unroll
              for (int ee = 0; ee < 10; ee++) B2[ee] = 0.0;
              int j2 = 0;
              for (int c = 0; c < C; c++) {
                const uint32_t k = pk.get(c);
                if (k != kNone) add_view(B2, c, k, j2++);
              }
              solve_and_score<!PERK, true, F32R>(cv, B2, v, obs_p, X2, e2);
              atomicAdd(&p.status[p.n_frames], 1);
              if (e2 <= bound) printf("EIGCHECK candidate: root %d g %u bound %.17g true %.17g\n", r, gl, bound, e2);
            }
#endif
          }
          // deliver: lexicographic minimum of (error bits, candidate index) in the (wave, root) slot; an error that is
          // not finite counts as +inf (such a candidate only ever stands when the root has no finite error at all);
          // the index word carries "the error was NaN" in its lowest bit (the error itself is not stored)
          const bool fin = e < inf;
          const unsigned long long key = fin ? (unsigned long long)__double_as_longlong(e) : kInfBits;
          const uint32_t gword = (gl << 1) | ((e != e) ? 1u : 0u);
          const int ss = wave * RS + r;
          if (fin) atomicMin(&rbound[r], key);
          const bool want = have && (key < slot_key[ss] || (key == slot_key[ss] && gword < slot_g[ss]));
          if (__ballot(want)) {
            unsigned long long old = 0;
            if (want) old = atomicMin(&slot_key[ss], key);
            wave_lds_sync();
            const bool holder = want && slot_key[ss] == key;
            if (holder && old > key) slot_g[ss] = 0xFFFFFFFFu;  // the error went down in this round: any index is better
            wave_lds_sync();
            if (holder) atomicMin(&slot_g[ss], gword);
            wave_lds_sync();
            // the lane that holds the slot after this round -- its error AND its index stood -- leaves the candidate's point and
            // its group's blob bytes in the slot's record of the workspace (phase E reads the winning slot's and nothing else of
            // the group); every change of a slot's (key, index) pair comes with the store of the lane that made it, a cut-short
            // or NaN candidate's included (it can be all a root has)
            // (a slot can be re-won by another lane of this wave in a later pass of this loop, with no barrier in between: the
            // record's words are stored by ONE lane per pass, every word goes to its own address from one wave, and a wave's
            // stores to an address reach L2 in the order it issued them -- so each word, the bytes' included, ends up as the
            // last holder left it)
            if (holder && slot_g[ss] == gword) store_winner(ss, X, pk);
          }
        }
        block_sync_lds_only();  // every lane is done with the records: new ones may be queued (through the other counter)
        pc_mark<PC_EVAL>();
        if (tid == 0) *ctr = 0;
        {
          int32_t* t = ctr;
          ctr = ctr_other;
          ctr_other = t;
        }
        continue;
      }
      if (!blocks_left) break;
      const uint32_t b = b0 + (uint32_t)tid;
      const uint32_t bw = b0 + (uint32_t)(wave * 64);
      b0 += T;
      int r = 0;
      if (bw < nblocks) r = root_of_block(bw, b < nblocks ? b : nblocks - 1);  // wave-uniform branch
      // The tests first, the pushes behind a barrier.  Every lane read the queue counter at the top of this iteration; a wave that
      // is through its tests early must not bump it before the slowest wave has read it -- that wave would see a different queue,
      // take the other branch of the flush decision and the workgroup would fall apart (a window of a few dozen instructions
      // when the cached blocks need no decode: found in round 5 as 1 wrong frame in ~10^4 with 2-candidate blocks).
      bool do_push = false;
      uint32_t gh = 0;
      Pk pk;
      pk.clear();
      if (b < nblocks) {
        gh = b - boff[r];
        if (gh != seedgh[r]) {
          double B[10], tr;
          bool survive = true;
          if (bound_tests && b < (uint32_t)ncache) {
            // the bound from the seed pass, folded into one float on the safe side (bb_fold.hpp); a block that survives -- a
            // handful per frame -- rebuilds its blob indices
            survive = !bb_fold_dropped(bcache[b], root_y(r));
            if (survive) block_pk(r, gh, pk);
          } else if (bound_tests) {
            const int v = block_matrix(r, gh, pk, B);
            if (v >= 2) {
              const double s1 = eigcut_s1_shifted(B, c0, tr);
              survive = !dropped(r, s1, tr);
            }
          } else {
            block_pk(r, gh, pk);
          }
          do_push = survive;
#ifdef MOCAP_DEBUG_EIGCHECK  // self-check build: EVERY candidate of a dropped block is evaluated in full against the bound it was dropped on
          if (!survive) {
            const double bound = __longlong_as_double((long long)rbound[r]);
            const uint32_t pl = bpl[r];
            for (uint32_t l = 0; l < pl; l++) {
              double B2[10], X2[3], e2 = inf;
              Pk pk2;
              const int v2 = group_matrix<true>(r, gh * pl + l, 0, B2, pk2);
              auto obs2 = [&](int c, double& x, double& y) -> bool {
                const uint32_t k = pk2.get(c);
                if (k == kNone) return false;
                const float2 w = bxy[grow(c, k)];
                x = (double)w.x;
                y = (double)w.y;
                return true;
              };
              solve_and_score<!PERK, true, F32R>(cv, B2, v2, obs2, X2, e2);
              atomicAdd(&p.status[p.n_frames + 1], 1);
              if (e2 <= bound) printf("EIGCHECK block: root %d block %u candidate %u bound %.17g true %.17g\n", r, gh, l, bound, e2);
            }
          }
#endif
        }
      }
      block_sync_lds_only();
      if (do_push) push_block(r, gh, pk);
      block_sync_lds_only();
      pc_mark<PC_TEST>();
    }
    wait_own_stores();  // the winners' records have reached L2 (stores are acknowledged from there) before any lane reads one
    __syncthreads();
  }

  // winner of root r (one with candidates): the (wave, root) slots merged -- its key (error bits), index word and the wave
  // whose slot it is (that slot's record holds the point); false: no candidate of the root was delivered
  __device__ __forceinline__ bool root_winner(int r, unsigned long long& kb, uint32_t& gw, int& wb) const {
    kb = ~0ull;
    gw = 0xFFFFFFFFu;
    wb = 0;
    for (int w = 0; w < W; w++) {
      const int s = w * RS + r;
      const unsigned long long k = slot_key[s];
      const uint32_t g = slot_g[s];
      if (k < kb || (k == kb && g < gw)) {
        kb = k;
        gw = g;
        wb = w;
      }
    }
    return kb != ~0ull;
  }

  // ---------------------------------------------------------------- phase E
  // The winners do not live in LDS (12 doubles per root and wave: 4.5 of the frame's 33.8 KB, the difference between four
  // and five frames per CU) and are not solved for a second time either: the lane that ends an evaluation round as the holder of
  // a (wave, root) slot leaves its candidate's point -- solve_and_score's own bits -- and the group's packed blob bytes (the
  // Packed it evaluated: one byte per camera, kNone = not in the group) in the slot's record of the workgroup's workspace
  // (search(), the delivery): 24 + 8 CW bytes per slot in memory the workgroup rewrites frame after frame, i.e. in L2.
  // Slots are per wave, so no two waves ever write the same record and the merge of the four slots picks the record with them.
  static constexpr uint32_t kRecBytes = bb_rec_bytes(CW);
  __device__ __forceinline__ unsigned char* winner_rec(int s) const {  // (a uniform base + a 32-bit lane offset: the address stays out of the vector registers)
    return p.ws + (size_t)blockIdx.x * p.ws_stride + (size_t)(kRecBytes * (uint32_t)s);
  }
  __device__ __forceinline__ void store_winner(int s, const double (&X)[3], const Pk& pk) const {
    unsigned long long* rec = (unsigned long long*)winner_rec(s);
    if constexpr (CW == 1) {
      // 32 bytes at a multiple of 32 (the workspace is 256-byte aligned, so is the stride): two 16-byte stores
      typedef unsigned long long rec2_t __attribute__((ext_vector_type(2)));
      const rec2_t lo = {(unsigned long long)__double_as_longlong(X[0]), (unsigned long long)__double_as_longlong(X[1])};
      const rec2_t hi = {(unsigned long long)__double_as_longlong(X[2]), pk.w[0]};
      ((rec2_t*)rec)[0] = lo;
      ((rec2_t*)rec)[1] = hi;
    } else {
      // 40 bytes at a multiple of 8: five 8-byte stores
#pragma unroll
      for (int k = 0; k < 3; k++) rec[k] = (unsigned long long)__double_as_longlong(X[k]);
#pragma unroll
      for (int k = 0; k < CW; k++) rec[3 + k] = pk.w[k];
    }
  }
  // two bytes of a group (low 16 bits of `two`) as two entries of a correspondence row: 0xFF -> -1, any other byte (a blob
  // index, <= 63) -> itself; bytes that are table rows: C ML (the only byte with bit 7 set) -> -1, any other -> its blob, row & (ML - 1)
  __device__ static __forceinline__ uint32_t row_word(uint32_t two) {
    const uint32_t x = (two & 0xFFu) | ((two & 0xFF00u) << 8);
    if constexpr (ROWS) {
      static_assert(!ROWS || kNone == 0x80u, "row_word: the record of zeros is the byte with bit 7 set");
      return (x & ((uint32_t)(ML - 1) * 0x00010001u)) | ((x >> 7) & 0x00010001u) * 0xFFFFu;
    }
    const uint32_t none = ((x + 0x00010001u) >> 8) & 0x00010001u;  // 1 where the byte was 0xFF
    return x | none * 0xFF00u;
  }
  // Phase E reads slot_key, slot_g and outslot of the frame's LDS state and nothing else: none of the matching's arrays
  // (nh, hits, root_cam, root_blob) and no divmod -- the row comes from the record's bytes.
  __device__ void write_point(int64_t frame, int r) const {
    const int C = cn();
    unsigned long long kb;
    uint32_t gw;
    int wv;
    if (!root_winner(r, kb, gw, wv)) return;
    const double e = kb != kInfBits ? __longlong_as_double((long long)kb)
                                    : ((gw & 1u) ? __longlong_as_double(0x7ff8000000000000ll) : __builtin_huge_val());
    const size_t o = (size_t)frame * R + outslot[r];
    // The record was written by a lane of wave wv of this workgroup during this frame's search and is complete in L2: every
    // wave waits for its stores' acknowledgements (which come from L2) before the barrier that ends search().  The workgroup
    // uses the same addresses for every frame, so the vector L1 may still hold the line as an EARLIER frame left it: the loads
    // are agent-scope atomics (sc1), which the hardware never serves from the vector L1 -- the guarantee the AMDGPU memory
    // model builds agent-scope coherence on -- and which therefore see what the XCD's L2 holds.  (The next frame's stores cannot
    // overtake these loads either: the frame's last barrier is behind a wait for them.)
    const unsigned long long* rec = (const unsigned long long*)winner_rec(wv * RS + r);
    unsigned long long w[3 + CW];
#pragma unroll
    for (int k = 0; k < 3 + CW; k++) w[k] = q_ld(rec + k);
    p.err[o] = e;
    const double X[3] = {__longlong_as_double((long long)w[0]), __longlong_as_double((long long)w[1]), __longlong_as_double((long long)w[2])};
    int16_t* co = p.corr + o * C;
    if constexpr (CT == 8) {
      // eight cameras: the row is 16 bytes at a multiple of 16 bytes from the array's start -- one store instead of eight
      // (the type says 2-byte alignment: the caller's array is int16_t, and global memory takes the access at any alignment)
      typedef uint32_t row_t __attribute__((ext_vector_type(4), aligned(2)));
      const uint32_t lo = (uint32_t)w[3], hi = (uint32_t)(w[3] >> 32);
      row_t v = {row_word(lo), row_word(lo >> 16), row_word(hi), row_word(hi >> 16)};
      *(row_t*)co = v;
    } else {
      for (int c = 0; c < C; c++) {
        const uint32_t k = (uint32_t)(w[3 + (CW == 1 ? 0 : c >> 3)] >> (8 * (c & 7))) & 0xFFu;
        co[c] = k == kNone ? (int16_t)-1 : (int16_t)(ROWS ? k & (uint32_t)(ML - 1) : k);
      }
    }
    store_point(p, o, X);  // incl. the fused world-coordinate epilogue (helpers.py:96-103)
  }
};

template <bool F32R, int CW, int CT, int ML, int RL>
__global__ __launch_bounds__(kBBThreads, bb_wg_per_cu(RL)) void frame_bb_kernel(FrameArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#define BB_STATE BBState<F32R, CW, CT, ML, RL>
#include "frame_bb_body.inc"
#undef BB_STATE
}

// The same search for rigs whose cameras have intrinsics of their own (every K plain, no two need be equal): BBState's PERK
// paths.  A kernel name of its own rather than a sixth template parameter: the identical-K instantiations keep their symbols.
template <bool F32R, int CW, int CT, int ML, int RL>
__global__ __launch_bounds__(kBBThreads, bb_wg_per_cu(RL)) void frame_bb_calib_kernel(FrameArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#define BB_STATE BBState<F32R, CW, CT, ML, RL, true>
#include "frame_bb_body.inc"
#undef BB_STATE
}

int frame_bb_wg_per_cu_cap(int C, int M, int R) { return bb_wg_per_cu(bb_fixed_slots(C, M, R)); }
// The winners' records (BBState::winner_rec): one point per (wave, root slot), sized for the largest layout whatever the call's
// is -- one size per context, so that no launch ever makes the workspace grow behind another that is still queued on it
// (the re-submit's second pass follows the first at once, with another layout).  40 KB per workgroup (255 slots of the two-word
// record); the part a layout touches (6 KB at 48 slots and one word) is rewritten frame after frame and stays in L2.
size_t frame_bb_ws_bytes(int) { return BBLayout::al(bb_rec_bytes(2) * (size_t)kBBWaves * 255, 256); }
static_assert(bb_wg_per_cu(48) <= kBBMaxWgPerCu && bb_wg_per_cu(64) <= kBBMaxWgPerCu && bb_wg_per_cu(0) <= kBBMaxWgPerCu, "frame_capi.hip sizes the workspace for kBBMaxWgPerCu workgroups per CU");

hipError_t launch_frame_bb(const FrameArgs& a, int grid, hipStream_t stream) {
  const size_t lds = frame_bb_lds_bytes(a.cv.C, a.M, a.K_max);
  if (!a.ws || a.ws_stride < bb_rec_bytes(bb_cw(a.cv.C)) * (size_t)kBBWaves * (size_t)frame_bb_root_slots(a.cv.C, a.M, a.K_max)) return hipErrorInvalidValue;  // the winners' records
  // the kernel addresses the tables from one base (BBCamTables): the block layout of mocap_set_cameras, whose Pq is 12 C
  // doubles for identical intrinsics and 12 C C otherwise
  const size_t nPq = a.cv.uniformK ? (size_t)12 * a.cv.C : (size_t)12 * a.cv.C * a.cv.C;
  if (a.cv.RT != a.cv.Pq + nPq || a.cv.K4 != a.cv.RT + 12 * a.cv.C || a.cv.F != a.cv.K4 + 4 * a.cv.C) return hipErrorInvalidValue;
  void (*k)(FrameArgs);
  const bool f32 = a.cv.f32_rounding != 0;
  const int fixed = bb_fixed_slots(a.cv.C, a.M, a.K_max);
  if (fixed && fixed != 48 && fixed != 64) return hipErrorInvalidValue;
  static_assert(bb_cw(8) == 1 && bb_cw(9) == 2 && bb_cw(16) == 2, "BB_PICK takes CW = 1 up to eight cameras, CW = 2 above");
#define BB_PICK(KERNEL)                                                                             \
  (fixed == 48       ? (f32 ? KERNEL<true, 1, 8, 16, 48> : KERNEL<false, 1, 8, 16, 48>)             \
   : fixed == 64     ? (f32 ? KERNEL<true, 1, 8, 16, 64> : KERNEL<false, 1, 8, 16, 64>)             \
   : a.cv.C == 8     ? (f32 ? KERNEL<true, 1, 8, 0, 0> : KERNEL<false, 1, 8, 0, 0>)                 \
   : a.cv.C <= 8     ? (f32 ? KERNEL<true, 1, 0, 0, 0> : KERNEL<false, 1, 0, 0, 0>)                 \
                     : (f32 ? KERNEL<true, 2, 0, 0, 0> : KERNEL<false, 2, 0, 0, 0>))
  k = a.cv.uniformK ? BB_PICK(frame_bb_kernel) : BB_PICK(frame_bb_calib_kernel);
#undef BB_PICK
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k, dim3(grid), dim3(kBBThreads), lds, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
