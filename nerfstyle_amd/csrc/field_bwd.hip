// Fused field backward, host side, and the fused-tracker instantiations of k_field_bwd (GOUT = false); the
// kernel itself is in field_bwd.h, the gradients-out instantiations in field_bwd_gout.hip.
#include "field_bwd.h"

extern "C" {

uint64_t nsr_field_backward_workspace_bytes(uint32_t M, int with_perm) {
    return with_perm ? (uint64_t)M * 16 * sizeof(float4) : 0;        // the [M][16] float4 encoder-gradient buffer
}

int nsr_field_backward(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *xyzs, uint32_t M,
                       const int32_t *m_dev, const float *grad_sigmas, const float *grad_rgbs, float *grad_tables,
                       float *grad_mlp, int train_density_table, int train_color_table, const void *feats,
                       const uint32_t *perm, void *workspace, nsr_stream_t stream) {
    if (M == 0) return NSR_OK;
    NSR_CHECK_PTR(desc); NSR_CHECK_PTR(tables); NSR_CHECK_PTR(mlp_params); NSR_CHECK_PTR(xyzs);
    NSR_CHECK_PTR(grad_sigmas); NSR_CHECK_PTR(grad_rgbs);
    if ((train_density_table || train_color_table) && grad_tables == nullptr) return NSR_ERR_INVALID_ARG;
    FieldBwdArgs b;
    uint32_t nblocks;
    const int st = field_fill_args(desc, b.f, M, nblocks);
    if (st != NSR_OK) return st;
    if ((uintptr_t)tables & 15u) return NSR_ERR_INVALID_ARG;
    // 4-wave workgroups, one wave per SIMD (each wave needs the 512-register budget): one
    // workgroup per CU is resident, each walks a contiguous range of tiles
    const uint32_t ntiles = (M + 15) / 16;
    nblocks = (ntiles + 3) / 4;
    if (nblocks > 256) nblocks = 256;
    b.f.tiles_per_block = (ntiles + nblocks - 1) / nblocks;
    b.f.tables = tables; b.f.params = mlp_params; b.f.xyzs = xyzs; b.f.m_dev = m_dev; b.f.sigmas = nullptr; b.f.rgbs = nullptr;
    const bool gout = perm != nullptr && (train_density_table || train_color_table);
    // `feats` given together with `perm` were written by nsr_field_forward in perm's order (tile-major): the gradients-out
    // kernel walks the same order; the fused tracker kernel walks the buffers and cannot use them (it re-gathers)
    if (perm != nullptr && !gout) feats = nullptr;
    b.f.feats = const_cast<void *>(feats);
    b.f.perm = (gout && feats != nullptr) ? perm : nullptr;
    b.gout = nullptr;
    if (gout) {
        if (workspace == nullptr || ((uintptr_t)workspace & 15u)) return NSR_ERR_INVALID_ARG;
        if (!nsr_table_scatter_supported(b.f.lv)) return NSR_ERR_UNSUPPORTED;   // grid too fine for the 10-bit blocks: call without perm
        b.gout = (float4 *)workspace;
    }
    if (feats && ((uintptr_t)feats & 15u)) return NSR_ERR_INVALID_ARG;
    b.grad_sigmas = grad_sigmas; b.grad_rgbs = grad_rgbs; b.grad_tables = grad_tables; b.grad_mlp = grad_mlp;
    b.train_density = train_density_table; b.train_color = train_color_table; b.nc = desc->num_classes;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(nblocks);
    if (!gout) return field_bwd_launch_variant<false>(b, desc->table_dtype, desc->compute_dtype, feats != nullptr, grid, s);
    const int st1 = nsr_field_bwd_launch_gout(b, desc->table_dtype, desc->compute_dtype, feats != nullptr, grid, s);
    if (st1 != NSR_OK) return st1;
    // second kernel: the table scatter in the permutation's order, many waves per CU
    return nsr_table_scatter_launch(b.f.lv, b.f.bmin, b.f.bsize, xyzs, perm, m_dev, M, workspace, grad_tables, train_density_table,
                                    train_color_table, s);
}

}   // extern "C"
