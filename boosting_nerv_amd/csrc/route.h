// route.h -- kernel selection of bnerv_conv_igemm as data.  conv.hip::bnerv_conv_route names the order of the
// families ONCE; the entry point switches on its answer, and the host queries (bnerv_conv_partial_rows, bnerv_conv_splitk_ws_bytes,
// bnerv_conv_family) and the paired launch (wgrad.hip) read the same answer.  Every family's translation unit exports a pure
// predicate `*_ok` ("this descriptor is mine": shape, mode, alignment, environment switches -- no device call) and a launcher that is
// only called after its predicate said yes.  Host only.
#pragma once
#include "conv_common.h"
#include "launch.h"
#include <type_traits>

// "this call cannot run here for a RESOURCE reason": the one late refusal a launcher may still return (convbf.hip: no scratch for the
// weight fragments).  Not a BNERV_E_* value, so a real error is never mistaken for it.
constexpr int BNERV_DECLINED = 1;

template <int V> using mode_c = std::integral_constant<int, V>;      // a mode as a type: the families' mode tables call f(mode_c<IN>{}, mode_c<EP>{}, ...)

// Split-K policy: layers with a long K loop and almost no spatial parallelism (the low-resolution data gradients: Cin = 750 or 1975 at
// 9x16 = 2 tiles) spread the input-channel chunks over work items.  Only for EP_PLAIN, out_s == 1, and only when the caller gave a workspace.
struct bnerv_split_plan { int ksplit, chunks_per_split; };

struct bnerv_conv_route_t {
    bnerv_conv_desc d;          // the descriptor as the kernels see it (IN_UNSHUFFLE with in_s == 1 is IN_PLAIN: same gather, faster staging)
    int family;                 // BNERV_CONV_FAM_*
    int th, tw;                 // tile of the family's grid: a sums epilogue writes one [B][2][Cout] row per tile (streaming families, which have
                                // no such epilogue, report the 8x32 grid of the persistent kernels)
    int vec;                    // conv_vec_ok(d)
    bnerv_split_plan split;     // {1, 0} unless the family splits K into d.partial
    size_t ws_bytes;            // what the family writes into an EP_PLAIN d.partial (split-K or stem slabs); 0: nothing
    int rows() const { return cdiv(d.H, th) * cdiv(d.W, tw); }
};
// `skip`: a family that declined late (BNERV_DECLINED) -- the route goes on behind it.  Dimensions must be positive.
bnerv_conv_route_t bnerv_conv_route(const bnerv_conv_desc& d, int skip = -1);          // conv.hip

// the host-side part of the persistent kernels' arguments (the launchers fill in their own item bookkeeping)
static inline bnerv_conv::KArgs bnerv_conv_kargs(const bnerv_conv_desc& d, int vec, bnerv_split_plan sp = {1, 0}) {
    bnerv_conv::KArgs ka{};
    ka.d = d;
    ka.tiles_x = cdiv(d.W, bnerv_conv::TW);
    ka.tiles_y = cdiv(d.H, bnerv_conv::TH);
    ka.vec = vec;
    ka.ksplit = sp.ksplit;
    ka.chunks_per_split = sp.chunks_per_split;
    return ka;
}

// ---- the families' predicates and launchers
bool bnerv_head3_ok(const bnerv_conv_desc& d);                                          // head3.hip: 3x3 head with 3 outputs (forward + tanh, data gradient)
int bnerv_head3_launch(hipStream_t st, const bnerv_conv_desc& d);
bool bnerv_stem_dgrad_ok(const bnerv_conv_desc& d);                                     // stem.hip: images of <= 256 pixels, long K; slabs in d.partial
size_t bnerv_stem_dgrad_ws_bytes(const bnerv_conv_desc& d);
int bnerv_stem_dgrad_slabs(const bnerv_conv_desc& d);
int bnerv_stem_dgrad_launch(hipStream_t st, const bnerv_conv_desc& d);
bool bnerv_convs_ok(const bnerv_conv_desc& d, int vec);                                 // convs.hip: the low-resolution stages, 4x16 tiles
namespace bnerv_convs { struct SArgs; }
constexpr int BNERV_CONVS_TH = 4, BNERV_CONVS_TW = 16;                                   // its tile (convs.hip asserts them against convs_body.h)
bnerv_convs::SArgs bnerv_convs_sargs(const bnerv_conv_desc& d);                         // the host-side part of its kernels' arguments
int bnerv_convs_nq(const bnerv_conv_desc& d);                                           // staged channel quads: 4, 8, 16, or 24 (the 96-channel form)
int bnerv_convs_launch(hipStream_t st, const bnerv_conv_desc& d);
bool bnerv_convbf_ok(const bnerv_conv_desc& d, int vec, int ksplit);                    // convbf.hip: the wide layers on split bf16
int bnerv_convbf_launch(hipStream_t st, const bnerv_conv_desc& d, bnerv_split_plan sp); // may return BNERV_DECLINED
bool bnerv_conv4_ok(const bnerv_conv::KArgs& ka);                                       // conv4.hip: <= 12-channel 3x3 layers on the 4x4x1 MFMA
int bnerv_conv4_launch(hipStream_t st, bnerv_conv::KArgs& ka);

// ---- the wide form of the paired launch (bnerv_conv_wgrad_pair form 3: convbf.hip's conv next to the wide split weight gradient)
namespace bnerv_wb { struct WArgs; struct BwPlan; }
struct bnerv_bfpair_plan { bool take; int slots, nr, ntb; };      // slots per XCD, blocks per role, cout tiles per conv block; 8 * slots slabs
bnerv_bfpair_plan bnerv_convbf_pair_plan(const bnerv_conv_desc& c, int vec, const bnerv_wgrad_desc& w, const bnerv_wb::BwPlan& bp);
int bnerv_convbf_pair_launch(hipStream_t st, const bnerv_conv_desc& c, const bnerv_wb::WArgs& wa, const bnerv_wb::BwPlan& bp, const bnerv_bfpair_plan& p);   // may return BNERV_DECLINED
