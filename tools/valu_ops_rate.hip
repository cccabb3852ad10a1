// valu_ops_rate.hip -- issue cost of the non-transcendental VALU ops of the sigmoid / pack sequences (round 5): plain and packed f32 add / fma,
// the two 16-bit packs, at one and four waves per SIMD; independent chains of 8 registers (no dependent back-to-back issue).
// Round 10 rows (profiles/r10_interior_slots.txt): the other instructions of the 16-lane HMC interior loop -- the 32- and 64-bit
// row_newbcast moves of the all-gather, the DPP adds of the reduce-scatter, s_nop 0, and v_pk_fma_f32 with its three register pairs
// at the same position mod 4 (one VGPR bank pair) against pairs spread over both positions (64-bit operands are even-aligned, so a
// pair starts at 0 or 2 mod 4: there is no third position).
// Round 13 rows (profiles/r13_loop_layout.txt): what ONE wave pays for where an 8-byte instruction starts.  Each body is one asm
// statement opened by .p2align 3, so the parity of every instruction in it is known.  "0 mod 8" / "4 mod 8": the same 128
// independent 8-byte instructions with one s_nop 0 behind / in front of them.  "k + x": one 4-byte x after every k v_pk_fma_f32
// (half of the packed instructions then start at 4 mod 8, the parity changes every k + 1 instructions); the same stream with the
// 8-byte encoding of x is its aligned twin.  Last, streams of the 4- and 8-byte encodings of the loop's lone instructions.
//   hipcc --offload-arch=gfx950 -O2 tools/valu_ops_rate.hip -o tools/bin/valu_ops_rate && tools/bin/valu_ops_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#define REP16(X) X X X X X X X X X X X X X X X X
typedef float f2 __attribute__((ext_vector_type(2)));
#define LR_PROBE_CLOBBERS "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135"
#define PKF(d, a, b) "v_pk_fma_f32 v[" #d "], v[" #a "], v[" #b "], v[" #d "]\n\t"
#define PK0 PKF(32:33, 64:65, 96:97)
#define PK1 PKF(36:37, 68:69, 100:101)
#define PK2 PKF(40:41, 72:73, 104:105)
#define PK3 PKF(44:45, 76:77, 108:109)
#define PK4 PKF(48:49, 80:81, 112:113)
#define PK5 PKF(52:53, 84:85, 116:117)
#define PK6 PKF(56:57, 88:89, 120:121)
#define PK7 PKF(60:61, 92:93, 124:125)
#define OP8(F) F(128) F(129) F(130) F(131) F(132) F(133) F(134) F(135)
#define DPA(r) "v_add_f32_dpp v" #r ", v" #r ", v" #r " row_mirror row_mask:0xf bank_mask:0xf\n\t"
#define FM3(r) "v_fma_f32 v" #r ", v" #r ", v" #r ", v" #r "\n\t"
#define AD4(r) "v_add_f32_e32 v" #r ", 1.0, v" #r "\n\t"
#define AD8(r) "v_add_f32_e64 v" #r ", 1.0, v" #r "\n\t"
#define EX4(r) "v_exp_f32_e32 v" #r ", v" #r "\n\t"
#define EX8(r) "v_exp_f32_e64 v" #r ", v" #r "\n\t"
#define RC4(r) "v_rcp_f32_e32 v" #r ", v" #r "\n\t"
#define RC8(r) "v_rcp_f32_e64 v" #r ", v" #r "\n\t"
#define SN4(r) "s_nop 0\n\t"
#define VN4(r) "v_nop\n\t"
#define VN8(r) "v_nop_e64\n\t"
// one x after every 1, 2 and 7 packed instructions (16, 12 and 16 instructions per repetition)
#define MIX1(X) PK0 X(128) PK1 X(129) PK2 X(130) PK3 X(131) PK4 X(132) PK5 X(133) PK6 X(134) PK7 X(135)
#define MIX2(X) PK0 PK1 X(128) PK2 PK3 X(129) PK4 PK5 X(130) PK6 PK7 X(131)
#define MIX7(X) PK0 PK1 PK2 PK3 PK4 PK5 PK6 X(128) PK7 PK0 PK1 PK2 PK3 PK4 PK5 X(129)
#define BODY(S) asm volatile(".p2align 3\n\t" REP16(S) ::: LR_PROBE_CLOBBERS)
template <int WHICH> __global__ void k(float* out, int iters) {
    float a0 = threadIdx.x * 1e-3f, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
    f2 p0 = {a0, a1}, p1 = {a2, a3}, p2 = {a4, a5}, p3 = {a6, a7}, p4 = {a1, a0}, p5 = {a3, a2}, p6 = {a5, a4}, p7 = {a7, a6};
    unsigned u0 = 0, u1 = 0, u2 = 0, u3 = 0, u4 = 0, u5 = 0, u6 = 0, u7 = 0;
    if (WHICH >= 11) asm volatile("v_mov_b32 v32, 1.0\n\tv_mov_b32 v33, 1.0\n\tv_mov_b32 v34, 1.0\n\tv_mov_b32 v35, 1.0\n\tv_mov_b32 v36, 1.0\n\tv_mov_b32 v37, 1.0\n\tv_mov_b32 v38, 1.0\n\tv_mov_b32 v39, 1.0\n\tv_mov_b32 v40, 1.0\n\tv_mov_b32 v41, 1.0\n\tv_mov_b32 v42, 1.0\n\tv_mov_b32 v43, 1.0\n\tv_mov_b32 v44, 1.0\n\tv_mov_b32 v45, 1.0\n\tv_mov_b32 v46, 1.0\n\tv_mov_b32 v47, 1.0\n\tv_mov_b32 v48, 1.0\n\tv_mov_b32 v49, 1.0\n\tv_mov_b32 v50, 1.0\n\tv_mov_b32 v51, 1.0\n\tv_mov_b32 v52, 1.0\n\tv_mov_b32 v53, 1.0\n\tv_mov_b32 v54, 1.0\n\tv_mov_b32 v55, 1.0\n\tv_mov_b32 v56, 1.0\n\tv_mov_b32 v57, 1.0\n\tv_mov_b32 v58, 1.0\n\tv_mov_b32 v59, 1.0\n\tv_mov_b32 v60, 1.0\n\tv_mov_b32 v61, 1.0\n\tv_mov_b32 v62, 1.0\n\tv_mov_b32 v63, 1.0\n\tv_mov_b32 v64, 1.0\n\tv_mov_b32 v65, 1.0\n\tv_mov_b32 v66, 1.0\n\tv_mov_b32 v67, 1.0\n\tv_mov_b32 v68, 1.0\n\tv_mov_b32 v69, 1.0\n\tv_mov_b32 v70, 1.0\n\tv_mov_b32 v71, 1.0\n\tv_mov_b32 v72, 1.0\n\tv_mov_b32 v73, 1.0\n\tv_mov_b32 v74, 1.0\n\tv_mov_b32 v75, 1.0\n\tv_mov_b32 v76, 1.0\n\tv_mov_b32 v77, 1.0\n\tv_mov_b32 v78, 1.0\n\tv_mov_b32 v79, 1.0\n\tv_mov_b32 v80, 1.0\n\tv_mov_b32 v81, 1.0\n\tv_mov_b32 v82, 1.0\n\tv_mov_b32 v83, 1.0\n\tv_mov_b32 v84, 1.0\n\tv_mov_b32 v85, 1.0\n\tv_mov_b32 v86, 1.0\n\tv_mov_b32 v87, 1.0\n\tv_mov_b32 v88, 1.0\n\tv_mov_b32 v89, 1.0\n\tv_mov_b32 v90, 1.0\n\tv_mov_b32 v91, 1.0\n\tv_mov_b32 v92, 1.0\n\tv_mov_b32 v93, 1.0\n\tv_mov_b32 v94, 1.0\n\tv_mov_b32 v95, 1.0\n\tv_mov_b32 v96, 1.0\n\tv_mov_b32 v97, 1.0\n\tv_mov_b32 v98, 1.0\n\tv_mov_b32 v99, 1.0\n\tv_mov_b32 v100, 1.0\n\tv_mov_b32 v101, 1.0\n\tv_mov_b32 v102, 1.0\n\tv_mov_b32 v103, 1.0\n\tv_mov_b32 v104, 1.0\n\tv_mov_b32 v105, 1.0\n\tv_mov_b32 v106, 1.0\n\tv_mov_b32 v107, 1.0\n\tv_mov_b32 v108, 1.0\n\tv_mov_b32 v109, 1.0\n\tv_mov_b32 v110, 1.0\n\tv_mov_b32 v111, 1.0\n\tv_mov_b32 v112, 1.0\n\tv_mov_b32 v113, 1.0\n\tv_mov_b32 v114, 1.0\n\tv_mov_b32 v115, 1.0\n\tv_mov_b32 v116, 1.0\n\tv_mov_b32 v117, 1.0\n\tv_mov_b32 v118, 1.0\n\tv_mov_b32 v119, 1.0\n\tv_mov_b32 v120, 1.0\n\tv_mov_b32 v121, 1.0\n\tv_mov_b32 v122, 1.0\n\tv_mov_b32 v123, 1.0\n\tv_mov_b32 v124, 1.0\n\tv_mov_b32 v125, 1.0\n\tv_mov_b32 v126, 1.0\n\tv_mov_b32 v127, 1.0\n\tv_mov_b32 v128, 1.0\n\tv_mov_b32 v129, 1.0\n\tv_mov_b32 v130, 1.0\n\tv_mov_b32 v131, 1.0\n\tv_mov_b32 v132, 1.0\n\tv_mov_b32 v133, 1.0\n\tv_mov_b32 v134, 1.0\n\tv_mov_b32 v135, 1.0" ::: LR_PROBE_CLOBBERS);
    for (int i = 0; i < iters; ++i) {
        if (WHICH == 0) { REP16(asm volatile("v_add_f32 %0, 1.0, %0\n\tv_add_f32 %1, 1.0, %1\n\tv_add_f32 %2, 1.0, %2\n\tv_add_f32 %3, 1.0, %3\n\tv_add_f32 %4, 1.0, %4\n\tv_add_f32 %5, 1.0, %5\n\tv_add_f32 %6, 1.0, %6\n\tv_add_f32 %7, 1.0, %7" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));) }
        if (WHICH == 1) { REP16(asm volatile("v_pk_add_f32 %0, %0, 1.0\n\tv_pk_add_f32 %1, %1, 1.0\n\tv_pk_add_f32 %2, %2, 1.0\n\tv_pk_add_f32 %3, %3, 1.0\n\tv_pk_add_f32 %4, %4, 1.0\n\tv_pk_add_f32 %5, %5, 1.0\n\tv_pk_add_f32 %6, %6, 1.0\n\tv_pk_add_f32 %7, %7, 1.0" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7));) }
        if (WHICH == 2) { REP16(asm volatile("v_pk_fma_f32 %0, %0, %0, %0\n\tv_pk_fma_f32 %1, %1, %1, %1\n\tv_pk_fma_f32 %2, %2, %2, %2\n\tv_pk_fma_f32 %3, %3, %3, %3\n\tv_pk_fma_f32 %4, %4, %4, %4\n\tv_pk_fma_f32 %5, %5, %5, %5\n\tv_pk_fma_f32 %6, %6, %6, %6\n\tv_pk_fma_f32 %7, %7, %7, %7" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7));) }
        if (WHICH == 3) { REP16(asm volatile("v_cvt_pk_bf16_f32 %0, %8, %9\n\tv_cvt_pk_bf16_f32 %1, %9, %10\n\tv_cvt_pk_bf16_f32 %2, %10, %11\n\tv_cvt_pk_bf16_f32 %3, %11, %12\n\tv_cvt_pk_bf16_f32 %4, %12, %13\n\tv_cvt_pk_bf16_f32 %5, %13, %14\n\tv_cvt_pk_bf16_f32 %6, %14, %15\n\tv_cvt_pk_bf16_f32 %7, %15, %8" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3), "+v"(u4), "+v"(u5), "+v"(u6), "+v"(u7) : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(a4), "v"(a5), "v"(a6), "v"(a7));) }
        if (WHICH == 4) { REP16(asm volatile("v_cvt_pk_f16_f32 %0, %8, %9\n\tv_cvt_pk_f16_f32 %1, %9, %10\n\tv_cvt_pk_f16_f32 %2, %10, %11\n\tv_cvt_pk_f16_f32 %3, %11, %12\n\tv_cvt_pk_f16_f32 %4, %12, %13\n\tv_cvt_pk_f16_f32 %5, %13, %14\n\tv_cvt_pk_f16_f32 %6, %14, %15\n\tv_cvt_pk_f16_f32 %7, %15, %8" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3), "+v"(u4), "+v"(u5), "+v"(u6), "+v"(u7) : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(a4), "v"(a5), "v"(a6), "v"(a7));) }
        if (WHICH == 5) { REP16(asm volatile("v_fma_f32 %0, %0, %0, %0\n\tv_fma_f32 %1, %1, %1, %1\n\tv_fma_f32 %2, %2, %2, %2\n\tv_fma_f32 %3, %3, %3, %3\n\tv_fma_f32 %4, %4, %4, %4\n\tv_fma_f32 %5, %5, %5, %5\n\tv_fma_f32 %6, %6, %6, %6\n\tv_fma_f32 %7, %7, %7, %7" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));) }
        if (WHICH == 6) { REP16(asm volatile("v_mov_b32_dpp %0, %0 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b32_dpp %1, %1 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b32_dpp %2, %2 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b32_dpp %3, %3 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b32_dpp %4, %4 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b32_dpp %5, %5 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b32_dpp %6, %6 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b32_dpp %7, %7 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));) }
        if (WHICH == 7) { REP16(asm volatile("v_mov_b64_dpp %0, %0 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b64_dpp %1, %1 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b64_dpp %2, %2 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b64_dpp %3, %3 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b64_dpp %4, %4 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b64_dpp %5, %5 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b64_dpp %6, %6 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_mov_b64_dpp %7, %7 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7));) }
        if (WHICH == 8) { REP16(asm volatile("v_add_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %1, %1, %1 row_mirror row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %2, %2, %2 row_mirror row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %3, %3, %3 row_mirror row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %4, %4, %4 row_mirror row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %5, %5, %5 row_mirror row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %6, %6, %6 row_mirror row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %7, %7, %7 row_mirror row_mask:0xf bank_mask:0xf" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));) }
        if (WHICH == 9) { REP16(asm volatile("v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %2, %2, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %3, %3, %3 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %4, %4, %4 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %5, %5, %5 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %6, %6, %6 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %7, %7, %7 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));) }
        if (WHICH == 10) { REP16(asm volatile("s_nop 0\n\ts_nop 0\n\ts_nop 0\n\ts_nop 0\n\ts_nop 0\n\ts_nop 0\n\ts_nop 0\n\ts_nop 0");) }
        // (fixed registers: accumulator pairs v[32+4k:33+4k], sources from v[64..] and v[96..]; LR_PROBE_CLOBBERS names all of them)
        if (WHICH == 11) { REP16(asm volatile("v_pk_fma_f32 v[32:33], v[64:65], v[96:97], v[32:33]\n\tv_pk_fma_f32 v[36:37], v[68:69], v[100:101], v[36:37]\n\tv_pk_fma_f32 v[40:41], v[72:73], v[104:105], v[40:41]\n\tv_pk_fma_f32 v[44:45], v[76:77], v[108:109], v[44:45]\n\tv_pk_fma_f32 v[48:49], v[80:81], v[112:113], v[48:49]\n\tv_pk_fma_f32 v[52:53], v[84:85], v[116:117], v[52:53]\n\tv_pk_fma_f32 v[56:57], v[88:89], v[120:121], v[56:57]\n\tv_pk_fma_f32 v[60:61], v[92:93], v[124:125], v[60:61]" ::: LR_PROBE_CLOBBERS);) }
        if (WHICH == 12) { REP16(asm volatile("v_pk_fma_f32 v[32:33], v[66:67], v[96:97], v[32:33]\n\tv_pk_fma_f32 v[36:37], v[70:71], v[100:101], v[36:37]\n\tv_pk_fma_f32 v[40:41], v[74:75], v[104:105], v[40:41]\n\tv_pk_fma_f32 v[44:45], v[78:79], v[108:109], v[44:45]\n\tv_pk_fma_f32 v[48:49], v[82:83], v[112:113], v[48:49]\n\tv_pk_fma_f32 v[52:53], v[86:87], v[116:117], v[52:53]\n\tv_pk_fma_f32 v[56:57], v[90:91], v[120:121], v[56:57]\n\tv_pk_fma_f32 v[60:61], v[94:95], v[124:125], v[60:61]" ::: LR_PROBE_CLOBBERS);) }
        if (WHICH == 13) { asm volatile(".p2align 3\n\t" REP16(PK0 PK1 PK2 PK3 PK4 PK5 PK6 PK7) "s_nop 0" ::: LR_PROBE_CLOBBERS); }
        if (WHICH == 14) { asm volatile(".p2align 3\n\ts_nop 0\n\t" REP16(PK0 PK1 PK2 PK3 PK4 PK5 PK6 PK7) ::: LR_PROBE_CLOBBERS); }
        if (WHICH == 15) { asm volatile(".p2align 3\n\t" REP16(OP8(DPA)) "s_nop 0" ::: LR_PROBE_CLOBBERS); }
        if (WHICH == 16) { asm volatile(".p2align 3\n\ts_nop 0\n\t" REP16(OP8(DPA)) ::: LR_PROBE_CLOBBERS); }
        if (WHICH == 17) { asm volatile(".p2align 3\n\t" REP16(OP8(FM3)) "s_nop 0" ::: LR_PROBE_CLOBBERS); }
        if (WHICH == 18) { asm volatile(".p2align 3\n\ts_nop 0\n\t" REP16(OP8(FM3)) ::: LR_PROBE_CLOBBERS); }
        if (WHICH == 19) { BODY(MIX1(EX4)); }
        if (WHICH == 20) { BODY(MIX1(EX8)); }
        if (WHICH == 21) { BODY(MIX1(SN4)); }
        if (WHICH == 22) { BODY(MIX1(VN8)); }
        if (WHICH == 23) { BODY(MIX2(EX4)); }
        if (WHICH == 24) { BODY(MIX2(EX8)); }
        if (WHICH == 25) { BODY(MIX2(SN4)); }
        if (WHICH == 26) { BODY(MIX2(VN8)); }
        if (WHICH == 27) { BODY(MIX7(EX4)); }
        if (WHICH == 28) { BODY(MIX7(EX8)); }
        if (WHICH == 29) { BODY(MIX7(SN4)); }
        if (WHICH == 30) { BODY(MIX7(VN8)); }
        if (WHICH == 31) { BODY(OP8(AD4)); }
        if (WHICH == 32) { BODY(OP8(AD8)); }
        if (WHICH == 33) { BODY(OP8(EX4)); }
        if (WHICH == 34) { BODY(OP8(EX8)); }
        if (WHICH == 35) { BODY(OP8(RC4)); }
        if (WHICH == 36) { BODY(OP8(RC8)); }
        if (WHICH == 37) { BODY(OP8(VN4)); }
        if (WHICH == 38) { BODY(OP8(VN8)); }
        if (WHICH == 39) { BODY(OP8(SN4)); }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + p0.x + p1.y + p2.x + p3.y + p4.x + p5.y + p6.x + p7.y + (float)(u0 ^ u1 ^ u2 ^ u3 ^ u4 ^ u5 ^ u6 ^ u7);
}
template <int W> void run(const char* name, int wps, int per_trip = 128) {
    float* d; hipMalloc(&d, 256 * 1024 * 64 * 4);
    const int iters = 2000, blocks = 256 * wps;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(k<W>, dim3(blocks), dim3(256), 0, 0, d, 10);
    hipEventRecord(e0); hipLaunchKernelGGL(k<W>, dim3(blocks), dim3(256), 0, 0, d, iters); hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("%-32s %d waves/SIMD: %.2f cycles@2.4GHz per wave-instruction per SIMD\n", name, wps, ms * 1e-3 * 2.4e9 / ((double)iters * per_trip * wps));
    hipFree(d);
}
int main() {
    for (int wps : {1, 2, 4}) {
        run<0>("v_add_f32", wps); run<5>("v_fma_f32", wps); run<1>("v_pk_add_f32", wps); run<2>("v_pk_fma_f32", wps);
        run<3>("v_cvt_pk_bf16_f32", wps); run<4>("v_cvt_pk_f16_f32", wps);
        run<6>("v_mov_b32_dpp newbcast", wps); run<7>("v_mov_b64_dpp newbcast", wps); run<8>("v_add_f32_dpp mirror", wps);
        run<9>("v_add_f32_dpp quad_perm", wps); run<10>("s_nop 0", wps); run<11>("v_pk_fma_f32 one bank", wps);
        run<12>("v_pk_fma_f32 two banks", wps);
        run<13>("v_pk_fma_f32 0 mod 8", wps, 129);
        run<14>("v_pk_fma_f32 4 mod 8", wps, 129);
        run<15>("v_add_f32_dpp 0 mod 8", wps, 129);
        run<16>("v_add_f32_dpp 4 mod 8", wps, 129);
        run<17>("v_fma_f32 (VOP3) 0 mod 8", wps, 129);
        run<18>("v_fma_f32 (VOP3) 4 mod 8", wps, 129);
        run<19>("1 pk_fma + v_exp_f32_e32", wps, 256);
        run<20>("1 pk_fma + v_exp_f32_e64", wps, 256);
        run<21>("1 pk_fma + s_nop 0", wps, 256);
        run<22>("1 pk_fma + v_nop_e64", wps, 256);
        run<23>("2 pk_fma + v_exp_f32_e32", wps, 192);
        run<24>("2 pk_fma + v_exp_f32_e64", wps, 192);
        run<25>("2 pk_fma + s_nop 0", wps, 192);
        run<26>("2 pk_fma + v_nop_e64", wps, 192);
        run<27>("7 pk_fma + v_exp_f32_e32", wps, 256);
        run<28>("7 pk_fma + v_exp_f32_e64", wps, 256);
        run<29>("7 pk_fma + s_nop 0", wps, 256);
        run<30>("7 pk_fma + v_nop_e64", wps, 256);
        run<31>("stream v_add_f32_e32", wps, 128);
        run<32>("stream v_add_f32_e64", wps, 128);
        run<33>("stream v_exp_f32_e32", wps, 128);
        run<34>("stream v_exp_f32_e64", wps, 128);
        run<35>("stream v_rcp_f32_e32", wps, 128);
        run<36>("stream v_rcp_f32_e64", wps, 128);
        run<37>("stream v_nop (e32)", wps, 128);
        run<38>("stream v_nop_e64", wps, 128);
        run<39>("stream s_nop 0 (aligned body)", wps, 128);
    }
    return 0;
}
