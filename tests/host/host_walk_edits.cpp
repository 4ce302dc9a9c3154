// host walk, relight edits: drn_gbuffer_edit_u8.  Sections A and D of the walk for this entry, in a file of its own: the family
// files that exist are left as they are.  The program's main() calls the families by name, so this one rides behind the picture
// family through the linker: tools/host_walk.py links with --wrap=_ZN2hw15family_picturesEv, which sends main()'s call of
// hw::family_pictures() to the function at the end of this file - the picture family itself first, then family_edits().
#include "host_walk.h"

namespace hw {
namespace {

const int64_t G = 1ll << 30;

// `maps` is a HOST table the library reads - a heap block of exactly n blocks, so ASan guards it
struct Ge { bool maps = 1, em = 1, im = 1, in_place = 0; int n = 5, null_src = -1, null_dst = -1, layers = 0x9, normal_at = 3, B = 2, T = 3, T_src = 3;
            int64_t px = 576 * 1024; int em_B = 2, em_T = 3, im_B = 2, im_T = 3, lay_B = 2, lay_T = 3;    // 1: that axis is broadcast
            int nan_gain = -1, inf_offset = -1, dst_is = 0;   // 1 edit_mask, 2 insert_mask, 3 map 0's layer, 4 the next map's src, 5 the next map's dst, 6 its own src a frame on
            int64_t src_ts_add = 0, dst_ts_add = 0, em_bs_add = 0; int mis = 0; };
int ge(const Ge& p) {
    const int64_t frame = p.px > 0 ? p.px * 3 : 0, mframe = p.px > 0 ? p.px : 0;
    const int64_t B = p.B > 0 ? p.B : 0, T = p.T > 0 ? p.T : 0;
    const int n = p.n > 0 ? p.n : 1;
    drn_gbuffer_edit_map* tab = p.maps ? new drn_gbuffer_edit_map[(size_t)n]() : nullptr;
    void* em = p.em ? A("edit_mask", p.em_B * p.em_T * mframe) : 0;
    void* im = p.im ? A("insert_mask", p.im_B * p.im_T * mframe) : 0;
    for (int k = 0; tab && k < n; ++k) {
        drn_gbuffer_edit_map& m = tab[k];
        m.src = k == p.null_src ? 0 : A("src", B * p.T_src * frame, p.mis);              // T_src > T: a [:, :T] view of a longer clip
        m.src_ts = frame + p.src_ts_add, m.src_bs = p.T_src * frame;
        m.dst = k == p.null_dst ? 0 : p.in_place ? (void*)m.src : A("dst", B * T * frame);
        m.dst_ts = (p.in_place ? m.src_ts : frame) + p.dst_ts_add, m.dst_bs = p.in_place ? m.src_bs : T * frame;
        if (p.layers >> k & 1) {
            m.layer = A("layer", p.lay_B * p.lay_T * frame);
            m.layer_ts = p.lay_T > 1 ? frame : 0, m.layer_bs = p.lay_B > 1 ? p.lay_T * frame : 0;
        }
        for (int c = 0; c < 3; ++c) m.gain[c] = k == 3 ? 1.f : 0.5f + (float)c, m.offset[c] = k == 3 ? 0.f : 7.25f - (float)k;
        if (k == p.nan_gain) m.gain[1] = __builtin_nanf("");
        if (k == p.inf_offset) m.offset[2] = -__builtin_inff();
        m.is_normal = k == p.normal_at;
    }
    if (tab && p.dst_is && n >= 2) {
        drn_gbuffer_edit_map& m = tab[0];
        if (p.dst_is == 1) m.dst = (char*)em + 5;
        if (p.dst_is == 2) m.dst = (char*)im + mframe - 1;
        if (p.dst_is == 3) m.dst = (char*)tab[0].layer + 16;
        if (p.dst_is == 4) m.dst = (char*)tab[1].src + frame;
        if (p.dst_is == 5) m.dst = (char*)tab[1].dst + 48;
        if (p.dst_is == 6) m.dst = (char*)m.src + frame;
    }
    const int rc = drn_gbuffer_edit_u8(tab, p.n, em, (p.em_B > 1 ? p.em_T * mframe : 0) + p.em_bs_add, p.em_T > 1 ? mframe : 0, im,
                                       p.im_B > 1 ? p.im_T * mframe : 0, p.im_T > 1 ? mframe : 0, p.B, p.T, p.px, STREAM);
    delete[] tab;
    return rc;
}

void family_edits() {
    entry<Ge>("drn_gbuffer_edit_u8", ge,
              {CH(Ge, "null maps", p.maps = 0), CH(Ge, "null src", p.null_src = 2), CH(Ge, "null dst", p.null_dst = 4), CH(Ge, "n_maps == 0", p.n = 0),
               CH(Ge, "n_maps == 6", p.n = 6), CH(Ge, "B == 0", p.B = 0), CH(Ge, "T < 0", p.T = -1), CH(Ge, "pixels < 0", p.px = -1),
               CH(Ge, "a layer without insert_mask", p.im = 0), CH(Ge, "a NaN gain", p.nan_gain = 1), CH(Ge, "an infinite offset", p.inf_offset = 4),
               CH(Ge, "dst inside edit_mask", p.dst_is = 1), CH(Ge, "dst over the end of insert_mask", p.dst_is = 2), CH(Ge, "dst inside a layer", p.dst_is = 3),
               CH(Ge, "dst inside another map's src", p.dst_is = 4), CH(Ge, "dst inside another map's dst", p.dst_is = 5),
               CH(Ge, "dst its own src a frame on", p.dst_is = 6), CH(Ge, "a negative stride", p.src_ts_add = -4 * 576 * 1024 * 3),
               CH(Ge, "dst frames that overlap", p.dst_ts_add = -16), CH(Ge, "B T pixels beyond 2^58", (p.B = 32768, p.T = 65536, p.px = 1ll << 28))},
              {CH(Ge, "pixels == 0", p.px = 0), CH(Ge, "in place", p.in_place = 1), CH(Ge, "in place on [:, :T] views of a longer clip", (p.in_place = 1, p.T_src = 9)),
               CH(Ge, "src a [:, :T] view, out of place", p.T_src = 9), CH(Ge, "masks broadcast over frames", (p.em_T = 1, p.im_T = 1)),
               CH(Ge, "masks broadcast over clips", (p.em_B = 1, p.im_B = 1)), CH(Ge, "masks and layers broadcast over both", (p.em_B = p.em_T = p.im_B = p.im_T = p.lay_B = p.lay_T = 1)),
               CH(Ge, "no edit_mask", p.em = 0), CH(Ge, "no layers, no insert_mask", (p.layers = 0, p.im = 0)), CH(Ge, "insert_mask without a layer", p.layers = 0),
               CH(Ge, "five layers", p.layers = 31), CH(Ge, "one map", p.n = 1), CH(Ge, "the normal map alone, with its layer", (p.n = 1, p.normal_at = 0, p.layers = 1)),
               CH(Ge, "src off the 16-byte grid", p.mis = 5), CH(Ge, "a mask stride off the 16-byte grid", p.em_bs_add = 4), CH(Ge, "one pixel", (p.px = 1, p.B = 1, p.T = 1, p.T_src = 1, p.em_B = p.em_T = p.im_B = p.im_T = p.lay_B = p.lay_T = 1)),
               CH(Ge, "pixels % 16 != 0", p.px = 1000003), CH(Ge, "57 frames of 576 x 1024", (p.B = 1, p.T = 57, p.T_src = 57, p.em_B = p.im_B = p.lay_B = 1, p.em_T = p.im_T = p.lay_T = 57)),
               // D: offsets beyond 32 bits
               CH(Ge, "a frame of 2^31 pixels", (p.px = 2 * G, p.B = 1, p.em_B = p.im_B = p.lay_B = 1)), CH(Ge, "a frame of 2^32 + 16 pixels, in place", (p.px = 4 * G + 16, p.in_place = 1)),
               CH(Ge, "2^31 frames of 16 pixels", (p.B = 32768, p.T = 65536, p.T_src = 65536, p.px = 16, p.em_B = p.im_B = p.lay_B = 1, p.em_T = p.im_T = p.lay_T = 1)),
               CH(Ge, "2^31 frames of 5 pixels, one per lane", (p.B = 65536, p.T = 32768, p.T_src = 32768, p.px = 5, p.em_B = p.im_B = p.lay_B = 1, p.em_T = p.im_T = p.lay_T = 1)),
               CH(Ge, "five maps of 48 GiB (~500 GB)", (p.B = 1, p.T = 1, p.T_src = 1, p.px = 16 * G, p.layers = 31, p.em_B = p.em_T = p.im_B = p.im_T = p.lay_B = p.lay_T = 1))});
}

}  // namespace
}  // namespace hw

// the linker's --wrap pair around hw::family_pictures() (the header of this file)
extern "C" void __real__ZN2hw15family_picturesEv();
extern "C" void __wrap__ZN2hw15family_picturesEv() {
    __real__ZN2hw15family_picturesEv();
    hw::family_edits();
}
