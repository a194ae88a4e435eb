// fft_team_list.h -- the device instantiations of team_fft_kernel (fft_team.h) and team_defer_kernel (fft_team_defer.h): four tiles per workgroup, sixteen
// (fp32) / eight (fp64) elements per thread, geometry baked in per (precision, log2 n).  MI355X: 8 XCDs x 32 CUs,
// 512-thread workgroups, 64 KiB tiles; a team is 2^(log2 n - 15) (fp32) / 2^(log2 n - 14) (fp64) CUs of one XCD.
#pragma once
#include "fft_team.h"

// THE list of built sizes: <T, log2 n, FFT_TEAM_GEO(log2 L1, log2 L2, log2 CA, log2 CB, log2 TS), ASPLIT, PAIR>.  What the planner takes for
// built (Pow2Plan::built_geo) and its dispatch (launch_team) come from it: a new size is one row.
//   ASPLIT: team_fft_kernel's variant with 128-byte column segments is instantiated too
//   PAIR:   so are team_defer_kernel's PAIR variants (paired row tiles, 128-byte result segments): the fp32 geometries with CB = 8 rows per row tile
#define FFT_TEAM_INSTANCES(X)                                                                   \
    X(float, 20, FFT_TEAM_GEO(10, 10, 3, 3, 5), true, true)   /* 1024 x 1024, whole XCD */      \
    X(float, 19, FFT_TEAM_GEO(9, 10, 4, 3, 4), false, true)   /*  512 x 1024, 16 CUs */         \
    X(float, 18, FFT_TEAM_GEO(9, 9, 4, 4, 3), false, false)   /*  512 x  512,  8 CUs */         \
    X(float, 17, FFT_TEAM_GEO(8, 9, 5, 4, 2), false, false)   /*  256 x  512,  4 CUs */         \
    X(float, 16, FFT_TEAM_GEO(8, 8, 5, 5, 1), false, false)   /*  256 x  256,  2 CUs */         \
    X(double, 19, FFT_TEAM_GEO(9, 10, 3, 2, 5), false, false)                                   \
    X(double, 18, FFT_TEAM_GEO(9, 9, 3, 3, 4), false, false)                                    \
    X(double, 17, FFT_TEAM_GEO(8, 9, 4, 3, 3), false, false)                                    \
    X(double, 16, FFT_TEAM_GEO(8, 8, 4, 4, 2), false, false)                                    \
    X(double, 15, FFT_TEAM_GEO(7, 8, 5, 4, 1), false, false)
