// nt_inst_stack.hip -- instantiates the view stack kernels of nt_stack.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 24: BoxScene's fused kernel box_stack<N>) and once with -DNT_INST_N=0: the kernels that take the dimension at
// run time (stack_cameras) or not at all (stack_resolve), and the three launchers nt_device.hpp declares.
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_stack.hpp"
#include "nt_dispatch.hpp"

#if NT_INST_N > 0

template <> int nt_box_stack<NT_INST_N>(const NtLaunchInfo &li, const NtTarget &tg, const NtStack &sk) {
    return launch_box_stack<NT_INST_N>(li, tg, sk);
}

#else

int nt_launch_stack_cameras(void *stream, int n, int nframes, const float *cams, const float *axes, const float *offsets, int count, float r,
                            float *out_cams, float *out_dots) {
    if (n < 3 || n > NT_DEV_MAX_DIM || nframes < 1 || count < 1 || count > NT_DEV_STACK_MAX || !cams || !axes || !offsets || !out_cams || !out_dots) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a view stack camera launch without its tables");
        return -1;
    }
    hipLaunchKernelGGL(stack_cameras, dim3((unsigned)nframes * (unsigned)count), dim3(64), 0, (hipStream_t)stream, n, count, cams, axes, offsets, r,
                       out_cams, out_dots);
    return finish_launch("view stack camera kernel launch");
}

int nt_launch_stack_resolve(void *stream, const NtStack &sk, const NtStackChunk &ch, const NtTarget &tg) {
    if (!ch.samples || ch.kc < 1 || ch.k0 < 0 || ch.k0 + ch.kc > sk.count || sk.count > NT_DEV_STACK_MAX || ch.nframes < 1 ||
        ((ch.acc_in || ch.acc_out) && ch.nframes != 1) || tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1 || tg.colors_out) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a view stack resolve launch that is not for whole frames, or beyond its samples");
        return -1;
    }
    const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + 3) / 4), (unsigned)ch.nframes);
    hipLaunchKernelGGL(stack_resolve, grid, dim3(256), 0, (hipStream_t)stream, tg, sk, ch);
    return finish_launch("view stack resolve kernel launch");
}

int nt_launch_box_stack(const NtLaunchInfo &li, const NtTarget &tg, const NtStack &sk) {
    int r = 0;
    if (!nt_dispatch_dim<3, NT_DEV_MAX_FIXED_BOX>(li.force_var ? 0 : li.n, r, [&](auto N) { return nt_box_stack<decltype(N)::value>(li, tg, sk); })) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: no fused view stack kernel at run-time n (n %d)", li.n);
        return -1;
    }
    if (r) return r;
    return finish_launch("view stack kernel launch");
}

#endif
