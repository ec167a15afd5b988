// nt_dispatch.hpp -- between the run-time dimension of a call and the compile-time-N launchers: the launchers' declarations
// and the one switch over n.  Standard headers only, so a host compiler builds it alone (tests/test_dispatch.py).
#pragma once
#include <type_traits>
#include <utility>

struct NtLaunchInfo;
struct NtCamera;
struct NtTarget;
struct NtCompositeDev;
struct NtQuery;
struct NtHits;
struct NtRayJob;
struct NtRefine;
struct NtLens;
struct NtParallel;
struct NtAo;
struct NtOutline;
struct NtCue;
struct NtBoxFaces;
struct NtBoxShade;
struct NtClip;
struct NtStack;
struct NtXray;
struct NtLayers;

// The compile-time-N launchers, one family a primary template.  Nothing defines the primary: every dimension is the explicit
// specialisation `template <> int nt_X_fixed<NT_INST_N>(...)` of its own translation unit (nt_inst_*.hip, compiled once per
// -DNT_INST_N), N = 3..NT_DEV_MAX_FIXED, and 3..NT_DEV_MAX_FIXED_BOX for box, rays_box and refine_box.
template <int N> int nt_box_fixed(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg);
template <int N> int nt_composite_fixed(const NtLaunchInfo &li, const NtCamera &cam, const NtCompositeDev &sc, const NtTarget &tg);
template <int N> int nt_query_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtQuery &q);
template <int N> int nt_hits_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtHits &h);
template <int N> int nt_rays_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtRayJob &job, const NtTarget &tg);
template <int N> int nt_rays_box_fixed(const NtLaunchInfo &li, const NtRayJob &job, const NtTarget &tg);
template <int N> int nt_refine_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtRefine &rf, const NtTarget &tg);
template <int N> int nt_refine_box_fixed(const NtLaunchInfo &li, const NtRefine &rf, const NtTarget &tg);
template <int N> int nt_lens_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtLens &ln);
template <int N> int nt_parallel_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtParallel &pl);
template <int N> int nt_ao_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtAo &ao);
template <int N> int nt_outline_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtOutline &ol, bool draw);
// (depth cues, nt_inst_cue.hip: N = 3..NT_DEV_MAX_FIXED like the others; the family is named for the walk it launches)
template <int N> int nt_cue_packet(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtCue &cu, bool draw);
// (clip planes, nt_inst_clip.hip: N = 3..NT_DEV_MAX_FIXED; named for the walk it launches, as the depth cues' family is)
template <int N> int nt_clip_packet(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtClip &cl, bool draw);
// (BoxScene hit buffers, nt_inst_boxhits.hip: N = 3..NT_DEV_MAX_FIXED_BOX like the other BoxScene families)
template <int N> int nt_box_faces(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg, const NtBoxFaces &bf);
// (BoxScene face shading, nt_inst_boxshade.hip: N = 3..NT_DEV_MAX_FIXED_BOX likewise)
template <int N> int nt_box_shade(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg, const NtBoxShade &bs);
// (view stacks, nt_inst_stack.hip: BoxScene's fused kernel, N = 3..NT_DEV_MAX_FIXED_BOX likewise)
template <int N> int nt_box_stack(const NtLaunchInfo &li, const NtTarget &tg, const NtStack &sk);
// (X-ray views, nt_inst_xray.hip: N = 3..NT_DEV_MAX_FIXED; named for the walk it launches, as the depth cues' family is)
template <int N> int nt_xray_packet(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtXray &xr);
// (hit layers, nt_inst_layers.hip: N = 3..NT_DEV_MAX_FIXED; named for the walk it launches likewise)
template <int N> int nt_layers_packet(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtLayers &ly);

template <int LO, typename F, int... I>
inline bool nt_dispatch_dim_seq(int n, int &r, F &f, std::integer_sequence<int, I...>) {
    return ((n == LO + I ? (r = f(std::integral_constant<int, LO + I>()), true) : false) || ...);
}

// n in [LO, HI]: r = f(std::integral_constant<int, n>()) -- one call, of the instantiation of that n -- and true; any other n:
// false, nothing called and r as it was.  A caller writes f as `[&](auto N) { return nt_X_fixed<decltype(N)::value>(...); }`.
template <int LO, int HI, typename F>
inline bool nt_dispatch_dim(int n, int &r, F &&f) {
    static_assert(LO <= HI, "empty range");
    return nt_dispatch_dim_seq<LO>(n, r, f, std::make_integer_sequence<int, HI - LO + 1>());
}
