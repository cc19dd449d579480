DEFINE_KERNEL(v_add_f32, "v_add_f32 %0, %0, %16\n v_add_f32 %1, %1, %16\n v_add_f32 %2, %2, %16\n v_add_f32 %3, %3, %16\n v_add_f32 %4, %4, %16\n v_add_f32 %5, %5, %16\n v_add_f32 %6, %6, %16\n v_add_f32 %7, %7, %16\n ")
DEFINE_KERNEL(v_add_f32_dep, "v_add_f32 %0, %0, %16\n v_add_f32 %0, %0, %16\n v_add_f32 %0, %0, %16\n v_add_f32 %0, %0, %16\n v_add_f32 %0, %0, %16\n v_add_f32 %0, %0, %16\n v_add_f32 %0, %0, %16\n v_add_f32 %0, %0, %16\n ")
DEFINE_KERNEL(v_sub_f32, "v_sub_f32 %0, %0, %16\n v_sub_f32 %1, %1, %16\n v_sub_f32 %2, %2, %16\n v_sub_f32 %3, %3, %16\n v_sub_f32 %4, %4, %16\n v_sub_f32 %5, %5, %16\n v_sub_f32 %6, %6, %16\n v_sub_f32 %7, %7, %16\n ")
DEFINE_KERNEL(v_mul_f32, "v_mul_f32 %0, %0, %16\n v_mul_f32 %1, %1, %16\n v_mul_f32 %2, %2, %16\n v_mul_f32 %3, %3, %16\n v_mul_f32 %4, %4, %16\n v_mul_f32 %5, %5, %16\n v_mul_f32 %6, %6, %16\n v_mul_f32 %7, %7, %16\n ")
DEFINE_KERNEL(v_fma_f32_2same, "v_fma_f32 %0, %0, %16, %16\n v_fma_f32 %1, %1, %16, %16\n v_fma_f32 %2, %2, %16, %16\n v_fma_f32 %3, %3, %16, %16\n v_fma_f32 %4, %4, %16, %16\n v_fma_f32 %5, %5, %16, %16\n v_fma_f32 %6, %6, %16, %16\n v_fma_f32 %7, %7, %16, %16\n ")
DEFINE_KERNEL(v_fma_f32_3distinct, "v_fma_f32 %0, %0, %16, %1\n v_fma_f32 %1, %1, %16, %2\n v_fma_f32 %2, %2, %16, %3\n v_fma_f32 %3, %3, %16, %4\n v_fma_f32 %4, %4, %16, %5\n v_fma_f32 %5, %5, %16, %6\n v_fma_f32 %6, %6, %16, %7\n v_fma_f32 %7, %7, %16, %0\n ")
DEFINE_KERNEL(v_fmac_f32, "v_fmac_f32 %0, %1, %16\n v_fmac_f32 %1, %2, %16\n v_fmac_f32 %2, %3, %16\n v_fmac_f32 %3, %4, %16\n v_fmac_f32 %4, %5, %16\n v_fmac_f32 %5, %6, %16\n v_fmac_f32 %6, %7, %16\n v_fmac_f32 %7, %0, %16\n ")
DEFINE_KERNEL(v_mac_like_mul_add, "v_mul_f32 %0, %0, %16\n v_mul_f32 %1, %1, %16\n v_mul_f32 %2, %2, %16\n v_mul_f32 %3, %3, %16\n v_mul_f32 %4, %4, %16\n v_mul_f32 %5, %5, %16\n v_mul_f32 %6, %6, %16\n v_mul_f32 %7, %7, %16\n ")
DEFINE_KERNEL(v_max_f32, "v_max_f32 %0, %0, %16\n v_max_f32 %1, %1, %16\n v_max_f32 %2, %2, %16\n v_max_f32 %3, %3, %16\n v_max_f32 %4, %4, %16\n v_max_f32 %5, %5, %16\n v_max_f32 %6, %6, %16\n v_max_f32 %7, %7, %16\n ")
DEFINE_KERNEL(v_min_f32, "v_min_f32 %0, %0, %16\n v_min_f32 %1, %1, %16\n v_min_f32 %2, %2, %16\n v_min_f32 %3, %3, %16\n v_min_f32 %4, %4, %16\n v_min_f32 %5, %5, %16\n v_min_f32 %6, %6, %16\n v_min_f32 %7, %7, %16\n ")
DEFINE_KERNEL(v_min3_f32, "v_min3_f32 %0, %0, %16, %1\n v_min3_f32 %1, %1, %16, %2\n v_min3_f32 %2, %2, %16, %3\n v_min3_f32 %3, %3, %16, %4\n v_min3_f32 %4, %4, %16, %5\n v_min3_f32 %5, %5, %16, %6\n v_min3_f32 %6, %6, %16, %7\n v_min3_f32 %7, %7, %16, %0\n ")
DEFINE_KERNEL(v_med3_f32, "v_med3_f32 %0, %0, %16, %1\n v_med3_f32 %1, %1, %16, %2\n v_med3_f32 %2, %2, %16, %3\n v_med3_f32 %3, %3, %16, %4\n v_med3_f32 %4, %4, %16, %5\n v_med3_f32 %5, %5, %16, %6\n v_med3_f32 %6, %6, %16, %7\n v_med3_f32 %7, %7, %16, %0\n ")
DEFINE_KERNEL(v_mov_b32, "v_mov_b32 %0, %1\n v_mov_b32 %1, %2\n v_mov_b32 %2, %3\n v_mov_b32 %3, %4\n v_mov_b32 %4, %5\n v_mov_b32 %5, %6\n v_mov_b32 %6, %7\n v_mov_b32 %7, %0\n ")
DEFINE_KERNEL(v_and_b32, "v_and_b32 %0, %0, %16\n v_and_b32 %1, %1, %16\n v_and_b32 %2, %2, %16\n v_and_b32 %3, %3, %16\n v_and_b32 %4, %4, %16\n v_and_b32 %5, %5, %16\n v_and_b32 %6, %6, %16\n v_and_b32 %7, %7, %16\n ")
DEFINE_KERNEL(v_or_b32, "v_or_b32 %0, %0, %16\n v_or_b32 %1, %1, %16\n v_or_b32 %2, %2, %16\n v_or_b32 %3, %3, %16\n v_or_b32 %4, %4, %16\n v_or_b32 %5, %5, %16\n v_or_b32 %6, %6, %16\n v_or_b32 %7, %7, %16\n ")
DEFINE_KERNEL(v_xor_b32, "v_xor_b32 %0, %0, %16\n v_xor_b32 %1, %1, %16\n v_xor_b32 %2, %2, %16\n v_xor_b32 %3, %3, %16\n v_xor_b32 %4, %4, %16\n v_xor_b32 %5, %5, %16\n v_xor_b32 %6, %6, %16\n v_xor_b32 %7, %7, %16\n ")
DEFINE_KERNEL(v_bfi_b32, "v_bfi_b32 %0, %0, %16, %1\n v_bfi_b32 %1, %1, %16, %2\n v_bfi_b32 %2, %2, %16, %3\n v_bfi_b32 %3, %3, %16, %4\n v_bfi_b32 %4, %4, %16, %5\n v_bfi_b32 %5, %5, %16, %6\n v_bfi_b32 %6, %6, %16, %7\n v_bfi_b32 %7, %7, %16, %0\n ")
DEFINE_KERNEL(v_and_or_b32, "v_and_or_b32 %0, %0, %16, %1\n v_and_or_b32 %1, %1, %16, %2\n v_and_or_b32 %2, %2, %16, %3\n v_and_or_b32 %3, %3, %16, %4\n v_and_or_b32 %4, %4, %16, %5\n v_and_or_b32 %5, %5, %16, %6\n v_and_or_b32 %6, %6, %16, %7\n v_and_or_b32 %7, %7, %16, %0\n ")
DEFINE_KERNEL(v_lshlrev_b32, "v_lshlrev_b32 %0, 3, %0\n v_lshlrev_b32 %1, 3, %1\n v_lshlrev_b32 %2, 3, %2\n v_lshlrev_b32 %3, 3, %3\n v_lshlrev_b32 %4, 3, %4\n v_lshlrev_b32 %5, 3, %5\n v_lshlrev_b32 %6, 3, %6\n v_lshlrev_b32 %7, 3, %7\n ")
DEFINE_KERNEL(v_lshrrev_b32, "v_lshrrev_b32 %0, 3, %0\n v_lshrrev_b32 %1, 3, %1\n v_lshrrev_b32 %2, 3, %2\n v_lshrrev_b32 %3, 3, %3\n v_lshrrev_b32 %4, 3, %4\n v_lshrrev_b32 %5, 3, %5\n v_lshrrev_b32 %6, 3, %6\n v_lshrrev_b32 %7, 3, %7\n ")
DEFINE_KERNEL(v_ashrrev_i32, "v_ashrrev_i32 %0, 31, %0\n v_ashrrev_i32 %1, 31, %1\n v_ashrrev_i32 %2, 31, %2\n v_ashrrev_i32 %3, 31, %3\n v_ashrrev_i32 %4, 31, %4\n v_ashrrev_i32 %5, 31, %5\n v_ashrrev_i32 %6, 31, %6\n v_ashrrev_i32 %7, 31, %7\n ")
DEFINE_KERNEL(v_bfe_i32, "v_bfe_i32 %0, %0, 0, 16\n v_bfe_i32 %1, %1, 0, 16\n v_bfe_i32 %2, %2, 0, 16\n v_bfe_i32 %3, %3, 0, 16\n v_bfe_i32 %4, %4, 0, 16\n v_bfe_i32 %5, %5, 0, 16\n v_bfe_i32 %6, %6, 0, 16\n v_bfe_i32 %7, %7, 0, 16\n ")
DEFINE_KERNEL(v_add_u32, "v_add_u32 %0, %0, %16\n v_add_u32 %1, %1, %16\n v_add_u32 %2, %2, %16\n v_add_u32 %3, %3, %16\n v_add_u32 %4, %4, %16\n v_add_u32 %5, %5, %16\n v_add_u32 %6, %6, %16\n v_add_u32 %7, %7, %16\n ")
DEFINE_KERNEL(v_sub_u32, "v_sub_u32 %0, %0, %16\n v_sub_u32 %1, %1, %16\n v_sub_u32 %2, %2, %16\n v_sub_u32 %3, %3, %16\n v_sub_u32 %4, %4, %16\n v_sub_u32 %5, %5, %16\n v_sub_u32 %6, %6, %16\n v_sub_u32 %7, %7, %16\n ")
DEFINE_KERNEL(v_add3_u32, "v_add3_u32 %0, %0, %16, %1\n v_add3_u32 %1, %1, %16, %2\n v_add3_u32 %2, %2, %16, %3\n v_add3_u32 %3, %3, %16, %4\n v_add3_u32 %4, %4, %16, %5\n v_add3_u32 %5, %5, %16, %6\n v_add3_u32 %6, %6, %16, %7\n v_add3_u32 %7, %7, %16, %0\n ")
DEFINE_KERNEL(v_lshl_add_u32, "v_lshl_add_u32 %0, %0, 2, %16\n v_lshl_add_u32 %1, %1, 2, %16\n v_lshl_add_u32 %2, %2, 2, %16\n v_lshl_add_u32 %3, %3, 2, %16\n v_lshl_add_u32 %4, %4, 2, %16\n v_lshl_add_u32 %5, %5, 2, %16\n v_lshl_add_u32 %6, %6, 2, %16\n v_lshl_add_u32 %7, %7, 2, %16\n ")
DEFINE_KERNEL(v_add_co_u32, "v_add_co_u32 %0, vcc, %0, %16\n v_add_co_u32 %1, vcc, %1, %16\n v_add_co_u32 %2, vcc, %2, %16\n v_add_co_u32 %3, vcc, %3, %16\n v_add_co_u32 %4, vcc, %4, %16\n v_add_co_u32 %5, vcc, %5, %16\n v_add_co_u32 %6, vcc, %6, %16\n v_add_co_u32 %7, vcc, %7, %16\n ")
DEFINE_KERNEL(v_addc_co_u32, "v_addc_co_u32 %0, vcc, %0, %16, vcc\n v_addc_co_u32 %1, vcc, %1, %16, vcc\n v_addc_co_u32 %2, vcc, %2, %16, vcc\n v_addc_co_u32 %3, vcc, %3, %16, vcc\n v_addc_co_u32 %4, vcc, %4, %16, vcc\n v_addc_co_u32 %5, vcc, %5, %16, vcc\n v_addc_co_u32 %6, vcc, %6, %16, vcc\n v_addc_co_u32 %7, vcc, %7, %16, vcc\n ")
DEFINE_KERNEL(v_mul_lo_u32, "v_mul_lo_u32 %0, %0, %16\n v_mul_lo_u32 %1, %1, %16\n v_mul_lo_u32 %2, %2, %16\n v_mul_lo_u32 %3, %3, %16\n v_mul_lo_u32 %4, %4, %16\n v_mul_lo_u32 %5, %5, %16\n v_mul_lo_u32 %6, %6, %16\n v_mul_lo_u32 %7, %7, %16\n ")
DEFINE_KERNEL(v_mul_u32_u24, "v_mul_u32_u24 %0, %0, %16\n v_mul_u32_u24 %1, %1, %16\n v_mul_u32_u24 %2, %2, %16\n v_mul_u32_u24 %3, %3, %16\n v_mul_u32_u24 %4, %4, %16\n v_mul_u32_u24 %5, %5, %16\n v_mul_u32_u24 %6, %6, %16\n v_mul_u32_u24 %7, %7, %16\n ")
DEFINE_KERNEL(v_mad_u32_u24, "v_mad_u32_u24 %0, %0, %16, %1\n v_mad_u32_u24 %1, %1, %16, %2\n v_mad_u32_u24 %2, %2, %16, %3\n v_mad_u32_u24 %3, %3, %16, %4\n v_mad_u32_u24 %4, %4, %16, %5\n v_mad_u32_u24 %5, %5, %16, %6\n v_mad_u32_u24 %6, %6, %16, %7\n v_mad_u32_u24 %7, %7, %16, %0\n ")
DEFINE_KERNEL(v_perm_b32, "v_perm_b32 %0, %0, %16, %1\n v_perm_b32 %1, %1, %16, %2\n v_perm_b32 %2, %2, %16, %3\n v_perm_b32 %3, %3, %16, %4\n v_perm_b32 %4, %4, %16, %5\n v_perm_b32 %5, %5, %16, %6\n v_perm_b32 %6, %6, %16, %7\n v_perm_b32 %7, %7, %16, %0\n ")
DEFINE_KERNEL(v_min_i32, "v_min_i32 %0, %0, %16\n v_min_i32 %1, %1, %16\n v_min_i32 %2, %2, %16\n v_min_i32 %3, %3, %16\n v_min_i32 %4, %4, %16\n v_min_i32 %5, %5, %16\n v_min_i32 %6, %6, %16\n v_min_i32 %7, %7, %16\n ")
DEFINE_KERNEL(v_max_u32, "v_max_u32 %0, %0, %16\n v_max_u32 %1, %1, %16\n v_max_u32 %2, %2, %16\n v_max_u32 %3, %3, %16\n v_max_u32 %4, %4, %16\n v_max_u32 %5, %5, %16\n v_max_u32 %6, %6, %16\n v_max_u32 %7, %7, %16\n ")
DEFINE_KERNEL(v_pk_add_f32, "v_pk_add_f32 %8, %8, %17\n v_pk_add_f32 %9, %9, %17\n v_pk_add_f32 %10, %10, %17\n v_pk_add_f32 %11, %11, %17\n v_pk_add_f32 %12, %12, %17\n v_pk_add_f32 %13, %13, %17\n v_pk_add_f32 %14, %14, %17\n v_pk_add_f32 %15, %15, %17\n ")
DEFINE_KERNEL(v_pk_mul_f32, "v_pk_mul_f32 %8, %8, %17\n v_pk_mul_f32 %9, %9, %17\n v_pk_mul_f32 %10, %10, %17\n v_pk_mul_f32 %11, %11, %17\n v_pk_mul_f32 %12, %12, %17\n v_pk_mul_f32 %13, %13, %17\n v_pk_mul_f32 %14, %14, %17\n v_pk_mul_f32 %15, %15, %17\n ")
DEFINE_KERNEL(v_pk_fma_f32, "v_pk_fma_f32 %8, %8, %17, %17\n v_pk_fma_f32 %9, %9, %17, %17\n v_pk_fma_f32 %10, %10, %17, %17\n v_pk_fma_f32 %11, %11, %17, %17\n v_pk_fma_f32 %12, %12, %17, %17\n v_pk_fma_f32 %13, %13, %17, %17\n v_pk_fma_f32 %14, %14, %17, %17\n v_pk_fma_f32 %15, %15, %17, %17\n ")
DEFINE_KERNEL(v_pk_mov_b32, "v_pk_mov_b32 %8, %9, %17\n v_pk_mov_b32 %9, %10, %17\n v_pk_mov_b32 %10, %11, %17\n v_pk_mov_b32 %11, %12, %17\n v_pk_mov_b32 %12, %13, %17\n v_pk_mov_b32 %13, %14, %17\n v_pk_mov_b32 %14, %15, %17\n v_pk_mov_b32 %15, %8, %17\n ")
DEFINE_KERNEL(v_pk_add_u16, "v_pk_add_u16 %0, %0, %16\n v_pk_add_u16 %1, %1, %16\n v_pk_add_u16 %2, %2, %16\n v_pk_add_u16 %3, %3, %16\n v_pk_add_u16 %4, %4, %16\n v_pk_add_u16 %5, %5, %16\n v_pk_add_u16 %6, %6, %16\n v_pk_add_u16 %7, %7, %16\n ")
DEFINE_KERNEL(v_pk_max_i16, "v_pk_max_i16 %0, %0, %16\n v_pk_max_i16 %1, %1, %16\n v_pk_max_i16 %2, %2, %16\n v_pk_max_i16 %3, %3, %16\n v_pk_max_i16 %4, %4, %16\n v_pk_max_i16 %5, %5, %16\n v_pk_max_i16 %6, %6, %16\n v_pk_max_i16 %7, %7, %16\n ")
DEFINE_KERNEL(v_add_f64, "v_add_f64 %8, %8, %17\n v_add_f64 %9, %9, %17\n v_add_f64 %10, %10, %17\n v_add_f64 %11, %11, %17\n v_add_f64 %12, %12, %17\n v_add_f64 %13, %13, %17\n v_add_f64 %14, %14, %17\n v_add_f64 %15, %15, %17\n ")
DEFINE_KERNEL(v_add_f64_dep, "v_add_f64 %8, %8, %17\n v_add_f64 %8, %8, %17\n v_add_f64 %8, %8, %17\n v_add_f64 %8, %8, %17\n v_add_f64 %8, %8, %17\n v_add_f64 %8, %8, %17\n v_add_f64 %8, %8, %17\n v_add_f64 %8, %8, %17\n ")
DEFINE_KERNEL(v_mul_f64, "v_mul_f64 %8, %8, %17\n v_mul_f64 %9, %9, %17\n v_mul_f64 %10, %10, %17\n v_mul_f64 %11, %11, %17\n v_mul_f64 %12, %12, %17\n v_mul_f64 %13, %13, %17\n v_mul_f64 %14, %14, %17\n v_mul_f64 %15, %15, %17\n ")
DEFINE_KERNEL(v_fma_f64, "v_fma_f64 %8, %8, %17, %17\n v_fma_f64 %9, %9, %17, %17\n v_fma_f64 %10, %10, %17, %17\n v_fma_f64 %11, %11, %17, %17\n v_fma_f64 %12, %12, %17, %17\n v_fma_f64 %13, %13, %17, %17\n v_fma_f64 %14, %14, %17, %17\n v_fma_f64 %15, %15, %17, %17\n ")
DEFINE_KERNEL(v_max_f64, "v_max_f64 %8, %8, %17\n v_max_f64 %9, %9, %17\n v_max_f64 %10, %10, %17\n v_max_f64 %11, %11, %17\n v_max_f64 %12, %12, %17\n v_max_f64 %13, %13, %17\n v_max_f64 %14, %14, %17\n v_max_f64 %15, %15, %17\n ")
DEFINE_KERNEL(v_lshlrev_b64, "v_lshlrev_b64 %8, 1, %8\n v_lshlrev_b64 %9, 1, %9\n v_lshlrev_b64 %10, 1, %10\n v_lshlrev_b64 %11, 1, %11\n v_lshlrev_b64 %12, 1, %12\n v_lshlrev_b64 %13, 1, %13\n v_lshlrev_b64 %14, 1, %14\n v_lshlrev_b64 %15, 1, %15\n ")
DEFINE_KERNEL(v_cvt_f64_f32, "v_cvt_f64_f32 %8, %0\n v_cvt_f64_f32 %9, %1\n v_cvt_f64_f32 %10, %2\n v_cvt_f64_f32 %11, %3\n v_cvt_f64_f32 %12, %4\n v_cvt_f64_f32 %13, %5\n v_cvt_f64_f32 %14, %6\n v_cvt_f64_f32 %15, %7\n ")
DEFINE_KERNEL(v_cvt_f32_f64, "v_cvt_f32_f64 %0, %8\n v_cvt_f32_f64 %1, %9\n v_cvt_f32_f64 %2, %10\n v_cvt_f32_f64 %3, %11\n v_cvt_f32_f64 %4, %12\n v_cvt_f32_f64 %5, %13\n v_cvt_f32_f64 %6, %14\n v_cvt_f32_f64 %7, %15\n ")
DEFINE_KERNEL(v_cvt_f32_i32, "v_cvt_f32_i32 %0, %1\n v_cvt_f32_i32 %1, %2\n v_cvt_f32_i32 %2, %3\n v_cvt_f32_i32 %3, %4\n v_cvt_f32_i32 %4, %5\n v_cvt_f32_i32 %5, %6\n v_cvt_f32_i32 %6, %7\n v_cvt_f32_i32 %7, %0\n ")
DEFINE_KERNEL(v_cvt_f32_u32, "v_cvt_f32_u32 %0, %1\n v_cvt_f32_u32 %1, %2\n v_cvt_f32_u32 %2, %3\n v_cvt_f32_u32 %3, %4\n v_cvt_f32_u32 %4, %5\n v_cvt_f32_u32 %5, %6\n v_cvt_f32_u32 %6, %7\n v_cvt_f32_u32 %7, %0\n ")
DEFINE_KERNEL(v_cvt_i32_f32, "v_cvt_i32_f32 %0, %1\n v_cvt_i32_f32 %1, %2\n v_cvt_i32_f32 %2, %3\n v_cvt_i32_f32 %3, %4\n v_cvt_i32_f32 %4, %5\n v_cvt_i32_f32 %5, %6\n v_cvt_i32_f32 %6, %7\n v_cvt_i32_f32 %7, %0\n ")
DEFINE_KERNEL(v_cvt_f32_ubyte0, "v_cvt_f32_ubyte0 %0, %1\n v_cvt_f32_ubyte0 %1, %2\n v_cvt_f32_ubyte0 %2, %3\n v_cvt_f32_ubyte0 %3, %4\n v_cvt_f32_ubyte0 %4, %5\n v_cvt_f32_ubyte0 %5, %6\n v_cvt_f32_ubyte0 %6, %7\n v_cvt_f32_ubyte0 %7, %0\n ")
DEFINE_KERNEL(v_cvt_f32_i32_sdwa_w0, "v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0\n v_cvt_f32_i32_sdwa %1, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0\n v_cvt_f32_i32_sdwa %2, sext(%3) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0\n v_cvt_f32_i32_sdwa %3, sext(%4) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0\n v_cvt_f32_i32_sdwa %4, sext(%5) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0\n v_cvt_f32_i32_sdwa %5, sext(%6) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0\n v_cvt_f32_i32_sdwa %6, sext(%7) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0\n v_cvt_f32_i32_sdwa %7, sext(%0) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0\n ")
DEFINE_KERNEL(v_cvt_f32_f16, "v_cvt_f32_f16 %0, %1\n v_cvt_f32_f16 %1, %2\n v_cvt_f32_f16 %2, %3\n v_cvt_f32_f16 %3, %4\n v_cvt_f32_f16 %4, %5\n v_cvt_f32_f16 %5, %6\n v_cvt_f32_f16 %6, %7\n v_cvt_f32_f16 %7, %0\n ")
DEFINE_KERNEL(v_cvt_f64_i32, "v_cvt_f64_i32 %8, %0\n v_cvt_f64_i32 %9, %1\n v_cvt_f64_i32 %10, %2\n v_cvt_f64_i32 %11, %3\n v_cvt_f64_i32 %12, %4\n v_cvt_f64_i32 %13, %5\n v_cvt_f64_i32 %14, %6\n v_cvt_f64_i32 %15, %7\n ")
DEFINE_KERNEL(v_rndne_f32, "v_rndne_f32 %0, %1\n v_rndne_f32 %1, %2\n v_rndne_f32 %2, %3\n v_rndne_f32 %3, %4\n v_rndne_f32 %4, %5\n v_rndne_f32 %5, %6\n v_rndne_f32 %6, %7\n v_rndne_f32 %7, %0\n ")
DEFINE_KERNEL(v_ldexp_f32, "v_ldexp_f32 %0, %0, 3\n v_ldexp_f32 %1, %1, 3\n v_ldexp_f32 %2, %2, 3\n v_ldexp_f32 %3, %3, 3\n v_ldexp_f32 %4, %4, 3\n v_ldexp_f32 %5, %5, 3\n v_ldexp_f32 %6, %6, 3\n v_ldexp_f32 %7, %7, 3\n ")
DEFINE_KERNEL(v_frexp_mant_f32, "v_frexp_mant_f32 %0, %1\n v_frexp_mant_f32 %1, %2\n v_frexp_mant_f32 %2, %3\n v_frexp_mant_f32 %3, %4\n v_frexp_mant_f32 %4, %5\n v_frexp_mant_f32 %5, %6\n v_frexp_mant_f32 %6, %7\n v_frexp_mant_f32 %7, %0\n ")
DEFINE_KERNEL(v_rsq_f32, "v_rsq_f32 %0, %0\n v_rsq_f32 %1, %1\n v_rsq_f32 %2, %2\n v_rsq_f32 %3, %3\n v_rsq_f32 %4, %4\n v_rsq_f32 %5, %5\n v_rsq_f32 %6, %6\n v_rsq_f32 %7, %7\n ")
DEFINE_KERNEL(v_rcp_f32, "v_rcp_f32 %0, %0\n v_rcp_f32 %1, %1\n v_rcp_f32 %2, %2\n v_rcp_f32 %3, %3\n v_rcp_f32 %4, %4\n v_rcp_f32 %5, %5\n v_rcp_f32 %6, %6\n v_rcp_f32 %7, %7\n ")
DEFINE_KERNEL(v_sqrt_f32, "v_sqrt_f32 %0, %0\n v_sqrt_f32 %1, %1\n v_sqrt_f32 %2, %2\n v_sqrt_f32 %3, %3\n v_sqrt_f32 %4, %4\n v_sqrt_f32 %5, %5\n v_sqrt_f32 %6, %6\n v_sqrt_f32 %7, %7\n ")
DEFINE_KERNEL(v_rsq_f64, "v_rsq_f64 %8, %8\n v_rsq_f64 %9, %9\n v_rsq_f64 %10, %10\n v_rsq_f64 %11, %11\n v_rsq_f64 %12, %12\n v_rsq_f64 %13, %13\n v_rsq_f64 %14, %14\n v_rsq_f64 %15, %15\n ")
DEFINE_KERNEL(v_rcp_f64, "v_rcp_f64 %8, %8\n v_rcp_f64 %9, %9\n v_rcp_f64 %10, %10\n v_rcp_f64 %11, %11\n v_rcp_f64 %12, %12\n v_rcp_f64 %13, %13\n v_rcp_f64 %14, %14\n v_rcp_f64 %15, %15\n ")
DEFINE_KERNEL(v_sqrt_f64, "v_sqrt_f64 %8, %8\n v_sqrt_f64 %9, %9\n v_sqrt_f64 %10, %10\n v_sqrt_f64 %11, %11\n v_sqrt_f64 %12, %12\n v_sqrt_f64 %13, %13\n v_sqrt_f64 %14, %14\n v_sqrt_f64 %15, %15\n ")
DEFINE_KERNEL(v_cmp_gt_f32_sgpr, "v_cmp_gt_f32 s[20:21], %0, %16\n v_cmp_gt_f32 s[22:23], %1, %16\n v_cmp_gt_f32 s[24:25], %2, %16\n v_cmp_gt_f32 s[26:27], %3, %16\n v_cmp_gt_f32 s[20:21], %4, %16\n v_cmp_gt_f32 s[22:23], %5, %16\n v_cmp_gt_f32 s[24:25], %6, %16\n v_cmp_gt_f32 s[26:27], %7, %16\n ")
DEFINE_KERNEL(v_cmp_gt_f32_vcc, "v_cmp_gt_f32 vcc, %0, %16\n v_cmp_gt_f32 vcc, %1, %16\n v_cmp_gt_f32 vcc, %2, %16\n v_cmp_gt_f32 vcc, %3, %16\n v_cmp_gt_f32 vcc, %4, %16\n v_cmp_gt_f32 vcc, %5, %16\n v_cmp_gt_f32 vcc, %6, %16\n v_cmp_gt_f32 vcc, %7, %16\n ")
DEFINE_KERNEL(v_cmp_lt_i32_vcc, "v_cmp_lt_i32 vcc, %0, %16\n v_cmp_lt_i32 vcc, %1, %16\n v_cmp_lt_i32 vcc, %2, %16\n v_cmp_lt_i32 vcc, %3, %16\n v_cmp_lt_i32 vcc, %4, %16\n v_cmp_lt_i32 vcc, %5, %16\n v_cmp_lt_i32 vcc, %6, %16\n v_cmp_lt_i32 vcc, %7, %16\n ")
DEFINE_KERNEL(v_cmp_gt_f64_vcc, "v_cmp_gt_f64 vcc, %8, %17\n v_cmp_gt_f64 vcc, %9, %17\n v_cmp_gt_f64 vcc, %10, %17\n v_cmp_gt_f64 vcc, %11, %17\n v_cmp_gt_f64 vcc, %12, %17\n v_cmp_gt_f64 vcc, %13, %17\n v_cmp_gt_f64 vcc, %14, %17\n v_cmp_gt_f64 vcc, %15, %17\n ")
DEFINE_KERNEL(v_cmp_class_f32, "v_cmp_class_f32 vcc, %0, %16\n v_cmp_class_f32 vcc, %1, %16\n v_cmp_class_f32 vcc, %2, %16\n v_cmp_class_f32 vcc, %3, %16\n v_cmp_class_f32 vcc, %4, %16\n v_cmp_class_f32 vcc, %5, %16\n v_cmp_class_f32 vcc, %6, %16\n v_cmp_class_f32 vcc, %7, %16\n ")
DEFINE_KERNEL(v_cndmask_e64_sgpr, "v_cndmask_b32 %0, %0, %16, s[20:21]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n v_cndmask_b32 %2, %2, %16, s[24:25]\n v_cndmask_b32 %3, %3, %16, s[26:27]\n v_cndmask_b32 %4, %4, %16, s[20:21]\n v_cndmask_b32 %5, %5, %16, s[22:23]\n v_cndmask_b32 %6, %6, %16, s[24:25]\n v_cndmask_b32 %7, %7, %16, s[26:27]\n ")
DEFINE_KERNEL(v_cndmask_e32_vcc, "v_cndmask_b32 %0, %0, %16, vcc\n v_cndmask_b32 %1, %1, %16, vcc\n v_cndmask_b32 %2, %2, %16, vcc\n v_cndmask_b32 %3, %3, %16, vcc\n v_cndmask_b32 %4, %4, %16, vcc\n v_cndmask_b32 %5, %5, %16, vcc\n v_cndmask_b32 %6, %6, %16, vcc\n v_cndmask_b32 %7, %7, %16, vcc\n ")
DEFINE_KERNEL(v_cndmask_e64_neg, "v_cndmask_b32 %0, -%0, %16, s[20:21]\n v_cndmask_b32 %1, -%1, %16, s[22:23]\n v_cndmask_b32 %2, -%2, %16, s[24:25]\n v_cndmask_b32 %3, -%3, %16, s[26:27]\n v_cndmask_b32 %4, -%4, %16, s[20:21]\n v_cndmask_b32 %5, -%5, %16, s[22:23]\n v_cndmask_b32 %6, -%6, %16, s[24:25]\n v_cndmask_b32 %7, -%7, %16, s[26:27]\n ")
DEFINE_KERNEL(cmp_vcc_then_cndmask_vcc_dep, "v_cmp_gt_f32 vcc, %0, %16\n v_cndmask_b32 %0, %0, %1, vcc\n v_cmp_gt_f32 vcc, %0, %16\n v_cndmask_b32 %0, %0, %1, vcc\n v_cmp_gt_f32 vcc, %0, %16\n v_cndmask_b32 %0, %0, %1, vcc\n v_cmp_gt_f32 vcc, %0, %16\n v_cndmask_b32 %0, %0, %1, vcc\n ")
DEFINE_KERNEL(sub_ashr_bfi_select_dep, "v_sub_f32 %2, %0, %16\n v_ashrrev_i32 %2, 31, %2\n v_bfi_b32 %0, %2, %1, %0\n v_sub_f32 %2, %0, %16\n v_ashrrev_i32 %2, 31, %2\n v_bfi_b32 %0, %2, %1, %0\n v_sub_f32 %2, %0, %16\n v_ashrrev_i32 %2, 31, %2\n ")
DEFINE_KERNEL(valu_add_salu_1to1, "v_add_f32 %0, %0, %16\n s_and_b64 s[20:21], s[22:23], s[24:25]\n v_add_f32 %1, %1, %16\n s_and_b64 s[20:21], s[22:23], s[24:25]\n v_add_f32 %2, %2, %16\n s_and_b64 s[20:21], s[22:23], s[24:25]\n v_add_f32 %3, %3, %16\n s_and_b64 s[20:21], s[22:23], s[24:25]\n ")
DEFINE_KERNEL(valu_add_salu_3to1, "v_add_f32 %0, %0, %16\n v_add_f32 %1, %1, %16\n v_add_f32 %2, %2, %16\n s_and_b64 s[20:21], s[22:23], s[24:25]\n v_add_f32 %3, %3, %16\n v_add_f32 %4, %4, %16\n v_add_f32 %5, %5, %16\n s_or_b64 s[22:23], s[20:21], s[24:25]\n ")
DEFINE_KERNEL(valu_f64_salu_1to1, "v_add_f64 %8, %8, %17\n s_and_b64 s[20:21], s[22:23], s[24:25]\n v_add_f64 %9, %9, %17\n s_and_b64 s[20:21], s[22:23], s[24:25]\n v_add_f64 %10, %10, %17\n s_and_b64 s[20:21], s[22:23], s[24:25]\n v_add_f64 %11, %11, %17\n s_and_b64 s[20:21], s[22:23], s[24:25]\n ")
DEFINE_KERNEL(valu_f64_salu_3to1, "v_add_f64 %8, %8, %17\n v_add_f64 %9, %9, %17\n v_add_f64 %10, %10, %17\n s_and_b64 s[20:21], s[22:23], s[24:25]\n v_add_f64 %11, %11, %17\n v_add_f64 %12, %12, %17\n v_add_f64 %13, %13, %17\n s_or_b64 s[22:23], s[20:21], s[24:25]\n ")
DEFINE_KERNEL(salu_only, "s_and_b64 s[20:21], s[22:23], s[24:25]\n s_or_b64 s[22:23], s[20:21], s[26:27]\n s_and_b64 s[20:21], s[22:23], s[24:25]\n s_or_b64 s[22:23], s[20:21], s[26:27]\n s_and_b64 s[20:21], s[22:23], s[24:25]\n s_or_b64 s[22:23], s[20:21], s[26:27]\n s_and_b64 s[20:21], s[22:23], s[24:25]\n s_or_b64 s[22:23], s[20:21], s[26:27]\n ")
DEFINE_KERNEL(mix_add_f32_add_f64, "v_add_f32 %0, %0, %16\n v_add_f64 %8, %8, %17\n v_add_f32 %1, %1, %16\n v_add_f64 %9, %9, %17\n v_add_f32 %2, %2, %16\n v_add_f64 %10, %10, %17\n v_add_f32 %3, %3, %16\n v_add_f64 %11, %11, %17\n ")
DEFINE_KERNEL(mix_cvt_fma_f64, "v_cvt_f64_f32 %8, %0\n v_fma_f64 %9, %9, %17, %17\n v_cvt_f32_f64 %1, %10\n v_fma_f64 %11, %11, %17, %17\n v_cvt_f64_f32 %12, %2\n v_fma_f64 %13, %13, %17, %17\n v_cvt_f32_f64 %3, %14\n v_fma_f64 %15, %15, %17, %17\n ")
DEFINE_KERNEL(add_f32_x7_ds_write_b64, "v_add_f32 %0, %0, %16\n v_add_f32 %1, %1, %16\n v_add_f32 %2, %2, %16\n ds_write_b64 %18, %8\n v_add_f32 %4, %4, %16\n v_add_f32 %5, %5, %16\n v_add_f32 %6, %6, %16\n v_add_f32 %7, %7, %16\n ")
DEFINE_KERNEL(add_f64_x7_ds_write_b128, "v_add_f64 %8, %8, %17\n v_add_f64 %9, %9, %17\n v_add_f64 %10, %10, %17\n ds_write_b64 %18, %8\n v_add_f64 %12, %12, %17\n v_add_f64 %13, %13, %17\n v_add_f64 %14, %14, %17\n v_add_f64 %15, %15, %17\n ")
DEFINE_KERNEL(exec_region_1valu, "s_mov_b64 s[22:23], 0x0f0f0f0f\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %0, %16\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %1, %16\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %2, %16\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %3, %16\n s_mov_b64 exec, s[20:21]\n ")
DEFINE_KERNEL(exec_region_1valu_salu_1to1, "s_mov_b64 s[22:23], 0x0f0f0f0f\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %0, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %1, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %2, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %3, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n ")
DEFINE_KERNEL(exec_region_1valu_gap_add, "s_mov_b64 s[22:23], 0x0f0f0f0f\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %0, %16\n s_mov_b64 exec, s[20:21]\n v_add_f32 %4, %4, %16\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %1, %16\n s_mov_b64 exec, s[20:21]\n v_add_f32 %5, %5, %16\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %2, %16\n s_mov_b64 exec, s[20:21]\n v_add_f32 %6, %6, %16\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %3, %16\n s_mov_b64 exec, s[20:21]\n v_add_f32 %7, %7, %16\n ")
DEFINE_KERNEL(exec_region_1valu_gap_add_salu_1to1, "s_mov_b64 s[22:23], 0x0f0f0f0f\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %0, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n v_add_f32 %4, %4, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %1, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n v_add_f32 %5, %5, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %2, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n v_add_f32 %6, %6, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %3, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n v_add_f32 %7, %7, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n ")
DEFINE_KERNEL(exec_region_2valu, "s_mov_b64 s[22:23], 0x0f0f0f0f\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %0, %16\n v_or_b32 %1, %1, %16\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %1, %16\n v_or_b32 %2, %2, %16\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %2, %16\n v_or_b32 %3, %3, %16\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %3, %16\n v_or_b32 %0, %0, %16\n s_mov_b64 exec, s[20:21]\n ")
DEFINE_KERNEL(exec_region_2valu_salu_1to1, "s_mov_b64 s[22:23], 0x0f0f0f0f\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %0, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %1, %1, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %1, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %2, %2, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %2, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %3, %3, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %3, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %0, %0, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n ")
DEFINE_KERNEL(exec_region_2valu_gap_add, "s_mov_b64 s[22:23], 0x0f0f0f0f\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %0, %16\n v_or_b32 %1, %1, %16\n s_mov_b64 exec, s[20:21]\n v_add_f32 %4, %4, %16\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %1, %16\n v_or_b32 %2, %2, %16\n s_mov_b64 exec, s[20:21]\n v_add_f32 %5, %5, %16\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %2, %16\n v_or_b32 %3, %3, %16\n s_mov_b64 exec, s[20:21]\n v_add_f32 %6, %6, %16\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %3, %16\n v_or_b32 %0, %0, %16\n s_mov_b64 exec, s[20:21]\n v_add_f32 %7, %7, %16\n ")
DEFINE_KERNEL(exec_region_2valu_gap_add_salu_1to1, "s_mov_b64 s[22:23], 0x0f0f0f0f\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %0, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %1, %1, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n v_add_f32 %4, %4, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %1, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %2, %2, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n v_add_f32 %5, %5, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %2, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %3, %3, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n v_add_f32 %6, %6, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %3, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %0, %0, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n v_add_f32 %7, %7, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n ")
DEFINE_KERNEL(exec_region_3valu, "s_mov_b64 s[22:23], 0x0f0f0f0f\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %0, %16\n v_or_b32 %1, %1, %16\n v_mov_b32 %2, %16\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %1, %16\n v_or_b32 %2, %2, %16\n v_mov_b32 %3, %16\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %2, %16\n v_or_b32 %3, %3, %16\n v_mov_b32 %0, %16\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %3, %16\n v_or_b32 %0, %0, %16\n v_mov_b32 %1, %16\n s_mov_b64 exec, s[20:21]\n ")
DEFINE_KERNEL(exec_region_3valu_salu_1to1, "s_mov_b64 s[22:23], 0x0f0f0f0f\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %0, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %1, %1, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_mov_b32 %2, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %1, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %2, %2, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_mov_b32 %3, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %2, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %3, %3, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_mov_b32 %0, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %3, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %0, %0, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_mov_b32 %1, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n ")
DEFINE_KERNEL(exec_region_3valu_gap_add, "s_mov_b64 s[22:23], 0x0f0f0f0f\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %0, %16\n v_or_b32 %1, %1, %16\n v_mov_b32 %2, %16\n s_mov_b64 exec, s[20:21]\n v_add_f32 %4, %4, %16\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %1, %16\n v_or_b32 %2, %2, %16\n v_mov_b32 %3, %16\n s_mov_b64 exec, s[20:21]\n v_add_f32 %5, %5, %16\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %2, %16\n v_or_b32 %3, %3, %16\n v_mov_b32 %0, %16\n s_mov_b64 exec, s[20:21]\n v_add_f32 %6, %6, %16\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %3, %16\n v_or_b32 %0, %0, %16\n v_mov_b32 %1, %16\n s_mov_b64 exec, s[20:21]\n v_add_f32 %7, %7, %16\n ")
DEFINE_KERNEL(exec_region_3valu_gap_add_salu_1to1, "s_mov_b64 s[22:23], 0x0f0f0f0f\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %0, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %1, %1, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_mov_b32 %2, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n v_add_f32 %4, %4, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %1, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %2, %2, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_mov_b32 %3, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n v_add_f32 %5, %5, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %2, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %3, %3, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_mov_b32 %0, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n v_add_f32 %6, %6, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_and_saveexec_b64 s[20:21], s[22:23]\n v_mov_b32 %3, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_or_b32 %0, %0, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_mov_b32 %1, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n s_mov_b64 exec, s[20:21]\n v_add_f32 %7, %7, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n ")
DEFINE_KERNEL(select_1valu, "s_mov_b64 s[22:23], 0x0f0f0f0f\n v_cndmask_b32 %0, %0, %16, s[22:23]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n ")
DEFINE_KERNEL(select_1valu_salu_1to1, "s_mov_b64 s[22:23], 0x0f0f0f0f\n v_cndmask_b32 %0, %0, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n ")
DEFINE_KERNEL(select_1valu_gap_add, "s_mov_b64 s[22:23], 0x0f0f0f0f\n v_cndmask_b32 %0, %0, %16, s[22:23]\n v_add_f32 %4, %4, %16\n v_cndmask_b32 %1, %1, %16, s[22:23]\n v_add_f32 %5, %5, %16\n v_cndmask_b32 %2, %2, %16, s[22:23]\n v_add_f32 %6, %6, %16\n v_cndmask_b32 %3, %3, %16, s[22:23]\n v_add_f32 %7, %7, %16\n ")
DEFINE_KERNEL(select_1valu_gap_add_salu_1to1, "s_mov_b64 s[22:23], 0x0f0f0f0f\n v_cndmask_b32 %0, %0, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_add_f32 %4, %4, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_add_f32 %5, %5, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_add_f32 %6, %6, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_add_f32 %7, %7, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n ")
DEFINE_KERNEL(select_2valu, "s_mov_b64 s[22:23], 0x0f0f0f0f\n v_cndmask_b32 %0, %0, %16, s[22:23]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n v_cndmask_b32 %0, %0, %16, s[22:23]\n ")
DEFINE_KERNEL(select_2valu_salu_1to1, "s_mov_b64 s[22:23], 0x0f0f0f0f\n v_cndmask_b32 %0, %0, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %0, %0, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n ")
DEFINE_KERNEL(select_2valu_gap_add, "s_mov_b64 s[22:23], 0x0f0f0f0f\n v_cndmask_b32 %0, %0, %16, s[22:23]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n v_add_f32 %4, %4, %16\n v_cndmask_b32 %1, %1, %16, s[22:23]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n v_add_f32 %5, %5, %16\n v_cndmask_b32 %2, %2, %16, s[22:23]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n v_add_f32 %6, %6, %16\n v_cndmask_b32 %3, %3, %16, s[22:23]\n v_cndmask_b32 %0, %0, %16, s[22:23]\n v_add_f32 %7, %7, %16\n ")
DEFINE_KERNEL(select_2valu_gap_add_salu_1to1, "s_mov_b64 s[22:23], 0x0f0f0f0f\n v_cndmask_b32 %0, %0, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_add_f32 %4, %4, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_add_f32 %5, %5, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_add_f32 %6, %6, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %0, %0, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_add_f32 %7, %7, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n ")
DEFINE_KERNEL(select_3valu, "s_mov_b64 s[22:23], 0x0f0f0f0f\n v_cndmask_b32 %0, %0, %16, s[22:23]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n v_cndmask_b32 %0, %0, %16, s[22:23]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n v_cndmask_b32 %0, %0, %16, s[22:23]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n ")
DEFINE_KERNEL(select_3valu_salu_1to1, "s_mov_b64 s[22:23], 0x0f0f0f0f\n v_cndmask_b32 %0, %0, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %0, %0, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %0, %0, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n ")
DEFINE_KERNEL(select_3valu_gap_add, "s_mov_b64 s[22:23], 0x0f0f0f0f\n v_cndmask_b32 %0, %0, %16, s[22:23]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n v_add_f32 %4, %4, %16\n v_cndmask_b32 %1, %1, %16, s[22:23]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n v_add_f32 %5, %5, %16\n v_cndmask_b32 %2, %2, %16, s[22:23]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n v_cndmask_b32 %0, %0, %16, s[22:23]\n v_add_f32 %6, %6, %16\n v_cndmask_b32 %3, %3, %16, s[22:23]\n v_cndmask_b32 %0, %0, %16, s[22:23]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n v_add_f32 %7, %7, %16\n ")
DEFINE_KERNEL(select_3valu_gap_add_salu_1to1, "s_mov_b64 s[22:23], 0x0f0f0f0f\n v_cndmask_b32 %0, %0, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_add_f32 %4, %4, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_add_f32 %5, %5, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %2, %2, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %0, %0, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_add_f32 %6, %6, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %3, %3, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %0, %0, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_cndmask_b32 %1, %1, %16, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_add_f32 %7, %7, %16\n s_and_b64 s[24:25], s[26:27], s[26:27]\n ")
DEFINE_KERNEL(v_addc_co_u32_vcc, "v_addc_co_u32 %0, vcc, %0, %0, vcc\n v_addc_co_u32 %1, vcc, %1, %1, vcc\n v_addc_co_u32 %2, vcc, %2, %2, vcc\n v_addc_co_u32 %3, vcc, %3, %3, vcc\n v_addc_co_u32 %4, vcc, %4, %4, vcc\n v_addc_co_u32 %5, vcc, %5, %5, vcc\n v_addc_co_u32 %6, vcc, %6, %6, vcc\n v_addc_co_u32 %7, vcc, %7, %7, vcc\n ")
DEFINE_KERNEL(v_addc_co_u32_e64_sgpr, "v_addc_co_u32_e64 %0, s[20:21], %0, %0, s[22:23]\n v_addc_co_u32_e64 %1, s[20:21], %1, %1, s[22:23]\n v_addc_co_u32_e64 %2, s[20:21], %2, %2, s[22:23]\n v_addc_co_u32_e64 %3, s[20:21], %3, %3, s[22:23]\n v_addc_co_u32_e64 %4, s[20:21], %4, %4, s[22:23]\n v_addc_co_u32_e64 %5, s[20:21], %5, %5, s[22:23]\n v_addc_co_u32_e64 %6, s[20:21], %6, %6, s[22:23]\n v_addc_co_u32_e64 %7, s[20:21], %7, %7, s[22:23]\n ")
DEFINE_KERNEL(v_addc_co_u32_e64_salu_1to1, "v_addc_co_u32_e64 %0, s[20:21], %0, %0, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_addc_co_u32_e64 %1, s[20:21], %1, %1, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_addc_co_u32_e64 %2, s[20:21], %2, %2, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n v_addc_co_u32_e64 %3, s[20:21], %3, %3, s[22:23]\n s_and_b64 s[24:25], s[26:27], s[26:27]\n ")
static const Test tests[] = {
    {"v_add_f32", k_v_add_f32, 8},
    {"v_add_f32_dep", k_v_add_f32_dep, 8},
    {"v_sub_f32", k_v_sub_f32, 8},
    {"v_mul_f32", k_v_mul_f32, 8},
    {"v_fma_f32_2same", k_v_fma_f32_2same, 8},
    {"v_fma_f32_3distinct", k_v_fma_f32_3distinct, 8},
    {"v_fmac_f32", k_v_fmac_f32, 8},
    {"v_mac_like_mul_add", k_v_mac_like_mul_add, 8},
    {"v_max_f32", k_v_max_f32, 8},
    {"v_min_f32", k_v_min_f32, 8},
    {"v_min3_f32", k_v_min3_f32, 8},
    {"v_med3_f32", k_v_med3_f32, 8},
    {"v_mov_b32", k_v_mov_b32, 8},
    {"v_and_b32", k_v_and_b32, 8},
    {"v_or_b32", k_v_or_b32, 8},
    {"v_xor_b32", k_v_xor_b32, 8},
    {"v_bfi_b32", k_v_bfi_b32, 8},
    {"v_and_or_b32", k_v_and_or_b32, 8},
    {"v_lshlrev_b32", k_v_lshlrev_b32, 8},
    {"v_lshrrev_b32", k_v_lshrrev_b32, 8},
    {"v_ashrrev_i32", k_v_ashrrev_i32, 8},
    {"v_bfe_i32", k_v_bfe_i32, 8},
    {"v_add_u32", k_v_add_u32, 8},
    {"v_sub_u32", k_v_sub_u32, 8},
    {"v_add3_u32", k_v_add3_u32, 8},
    {"v_lshl_add_u32", k_v_lshl_add_u32, 8},
    {"v_add_co_u32", k_v_add_co_u32, 8},
    {"v_addc_co_u32", k_v_addc_co_u32, 8},
    {"v_mul_lo_u32", k_v_mul_lo_u32, 8},
    {"v_mul_u32_u24", k_v_mul_u32_u24, 8},
    {"v_mad_u32_u24", k_v_mad_u32_u24, 8},
    {"v_perm_b32", k_v_perm_b32, 8},
    {"v_min_i32", k_v_min_i32, 8},
    {"v_max_u32", k_v_max_u32, 8},
    {"v_pk_add_f32", k_v_pk_add_f32, 8},
    {"v_pk_mul_f32", k_v_pk_mul_f32, 8},
    {"v_pk_fma_f32", k_v_pk_fma_f32, 8},
    {"v_pk_mov_b32", k_v_pk_mov_b32, 8},
    {"v_pk_add_u16", k_v_pk_add_u16, 8},
    {"v_pk_max_i16", k_v_pk_max_i16, 8},
    {"v_add_f64", k_v_add_f64, 8},
    {"v_add_f64_dep", k_v_add_f64_dep, 8},
    {"v_mul_f64", k_v_mul_f64, 8},
    {"v_fma_f64", k_v_fma_f64, 8},
    {"v_max_f64", k_v_max_f64, 8},
    {"v_lshlrev_b64", k_v_lshlrev_b64, 8},
    {"v_cvt_f64_f32", k_v_cvt_f64_f32, 8},
    {"v_cvt_f32_f64", k_v_cvt_f32_f64, 8},
    {"v_cvt_f32_i32", k_v_cvt_f32_i32, 8},
    {"v_cvt_f32_u32", k_v_cvt_f32_u32, 8},
    {"v_cvt_i32_f32", k_v_cvt_i32_f32, 8},
    {"v_cvt_f32_ubyte0", k_v_cvt_f32_ubyte0, 8},
    {"v_cvt_f32_i32_sdwa_w0", k_v_cvt_f32_i32_sdwa_w0, 8},
    {"v_cvt_f32_f16", k_v_cvt_f32_f16, 8},
    {"v_cvt_f64_i32", k_v_cvt_f64_i32, 8},
    {"v_rndne_f32", k_v_rndne_f32, 8},
    {"v_ldexp_f32", k_v_ldexp_f32, 8},
    {"v_frexp_mant_f32", k_v_frexp_mant_f32, 8},
    {"v_rsq_f32", k_v_rsq_f32, 8},
    {"v_rcp_f32", k_v_rcp_f32, 8},
    {"v_sqrt_f32", k_v_sqrt_f32, 8},
    {"v_rsq_f64", k_v_rsq_f64, 8},
    {"v_rcp_f64", k_v_rcp_f64, 8},
    {"v_sqrt_f64", k_v_sqrt_f64, 8},
    {"v_cmp_gt_f32_sgpr", k_v_cmp_gt_f32_sgpr, 8},
    {"v_cmp_gt_f32_vcc", k_v_cmp_gt_f32_vcc, 8},
    {"v_cmp_lt_i32_vcc", k_v_cmp_lt_i32_vcc, 8},
    {"v_cmp_gt_f64_vcc", k_v_cmp_gt_f64_vcc, 8},
    {"v_cmp_class_f32", k_v_cmp_class_f32, 8},
    {"v_cndmask_e64_sgpr", k_v_cndmask_e64_sgpr, 8},
    {"v_cndmask_e32_vcc", k_v_cndmask_e32_vcc, 8},
    {"v_cndmask_e64_neg", k_v_cndmask_e64_neg, 8},
    {"cmp_vcc_then_cndmask_vcc_dep", k_cmp_vcc_then_cndmask_vcc_dep, 8},
    {"sub_ashr_bfi_select_dep", k_sub_ashr_bfi_select_dep, 8},
    {"valu_add_salu_1to1", k_valu_add_salu_1to1, 4},
    {"valu_add_salu_3to1", k_valu_add_salu_3to1, 6},
    {"valu_f64_salu_1to1", k_valu_f64_salu_1to1, 4},
    {"valu_f64_salu_3to1", k_valu_f64_salu_3to1, 6},
    {"salu_only", k_salu_only, 0},
    {"mix_add_f32_add_f64", k_mix_add_f32_add_f64, 8},
    {"mix_cvt_fma_f64", k_mix_cvt_fma_f64, 8},
    {"add_f32_x7_ds_write_b64", k_add_f32_x7_ds_write_b64, 7},
    {"add_f64_x7_ds_write_b128", k_add_f64_x7_ds_write_b128, 7},
    {"exec_region_1valu", k_exec_region_1valu, 4},
    {"exec_region_1valu_salu_1to1", k_exec_region_1valu_salu_1to1, 4},
    {"exec_region_1valu_gap_add", k_exec_region_1valu_gap_add, 8},
    {"exec_region_1valu_gap_add_salu_1to1", k_exec_region_1valu_gap_add_salu_1to1, 8},
    {"exec_region_2valu", k_exec_region_2valu, 8},
    {"exec_region_2valu_salu_1to1", k_exec_region_2valu_salu_1to1, 8},
    {"exec_region_2valu_gap_add", k_exec_region_2valu_gap_add, 12},
    {"exec_region_2valu_gap_add_salu_1to1", k_exec_region_2valu_gap_add_salu_1to1, 12},
    {"exec_region_3valu", k_exec_region_3valu, 12},
    {"exec_region_3valu_salu_1to1", k_exec_region_3valu_salu_1to1, 12},
    {"exec_region_3valu_gap_add", k_exec_region_3valu_gap_add, 16},
    {"exec_region_3valu_gap_add_salu_1to1", k_exec_region_3valu_gap_add_salu_1to1, 16},
    {"select_1valu", k_select_1valu, 4},
    {"select_1valu_salu_1to1", k_select_1valu_salu_1to1, 4},
    {"select_1valu_gap_add", k_select_1valu_gap_add, 8},
    {"select_1valu_gap_add_salu_1to1", k_select_1valu_gap_add_salu_1to1, 8},
    {"select_2valu", k_select_2valu, 8},
    {"select_2valu_salu_1to1", k_select_2valu_salu_1to1, 8},
    {"select_2valu_gap_add", k_select_2valu_gap_add, 12},
    {"select_2valu_gap_add_salu_1to1", k_select_2valu_gap_add_salu_1to1, 12},
    {"select_3valu", k_select_3valu, 12},
    {"select_3valu_salu_1to1", k_select_3valu_salu_1to1, 12},
    {"select_3valu_gap_add", k_select_3valu_gap_add, 16},
    {"select_3valu_gap_add_salu_1to1", k_select_3valu_gap_add_salu_1to1, 16},
    {"v_addc_co_u32_vcc", k_v_addc_co_u32_vcc, 8},
    {"v_addc_co_u32_e64_sgpr", k_v_addc_co_u32_e64_sgpr, 8},
    {"v_addc_co_u32_e64_salu_1to1", k_v_addc_co_u32_e64_salu_1to1, 4},
};
