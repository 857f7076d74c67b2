// The X-macro tables that decide which tile edges get which kernel family. Each table sits behind one #ifndef, so a
// development build can override it with -D; -DDCTS_DEV_FAST selects the short built-in tables (a handful of
// instantiations, seconds instead of minutes).
#pragma once

// Tile edge lengths that get a register-resident codelet kernel (edges AFTER the cv2-style
// odd front pad). Sources: SURVEY.md Appendix C — VGG 32/16/8/4/2, ResNet-56/110 and
// DenseNet 32/16/8, GoogLeNet 32/16/8, ResNet-50 56/28/14/7, U2-Net-p 36/18/9 (+10 via
// the odd pad) and its 320-crop family 40/20/10; 64 and 48 are the natural power-of-two /
// 3*2^k fillers; round 3 adds the remaining even edges below 64 whose odd part is 3 or 15 (6, 12, 24, 30, 60 - and with
// them 5, 11, 23, 29, 59 through the odd front pad), so that an --input_size other than 224 / 288 / 320 does not
// drop small maps to the cosine-matrix kernel.
#ifndef DCTS_CODELET_SIZES
#ifdef DCTS_DEV_FAST
#define DCTS_CODELET_SIZES(X) X(7) X(8) X(9) X(14) X(28) X(56)
#else
#define DCTS_CODELET_SIZES(X) \
  X(2) X(4) X(6) X(7) X(8) X(9) X(10) X(12) X(14) X(16) X(18) X(20) X(24) X(28) X(30) X(32) X(36) X(40) X(48) X(56) X(60) X(64)
#endif
#endif

// tile edges served by the split family: X(N, M, L) with N = M << L. L = 3 (eight M-point roles)
// where the four-role codelets would be too register-hungry for more than 1-2 waves per SIMD.
#ifndef DCTS_SPLIT_TABLE
#ifdef DCTS_DEV_FAST
#define DCTS_SPLIT_TABLE(X) X(128, 32, 2) X(224, 28, 3)
#else
// Round 3: the other multiples of 4 up to 256 (N = 4 * M) and of 8 up to 512 (N = 8 * M) with M <= 64 even or M <= 32 - the
// codelet template factorises any M; an odd M beyond 32 would be a direct M x M sum per leaf: minutes of build time each and
// compute-bound. These edges (an --input_size such as 272 / 304 / 352 / 384 / 448 / 512 and their halves) have no single-launch
// kernel: they take the two-launch path (3 x the algorithmic traffic: <= 0.2 of the HBM peak) instead of the cosine-matrix kernel
// (< 0.01). The 8 * M entries are a translation unit of their own (split_more.hip).
#define DCTS_SPLIT_TABLE_MORE_A(X) \
  X(68, 17, 2) X(76, 19, 2) X(84, 21, 2) X(88, 22, 2) X(92, 23, 2) X(100, 25, 2) X(104, 26, 2) \
  X(108, 27, 2) X(116, 29, 2) X(120, 30, 2) X(124, 31, 2) X(136, 34, 2) X(152, 38, 2) X(168, 42, 2) \
  X(176, 44, 2) X(184, 46, 2) X(200, 50, 2) X(208, 52, 2) X(216, 54, 2) X(232, 58, 2) X(240, 60, 2) \
  X(248, 62, 2)
#define DCTS_SPLIT_TABLE_MORE_B(X) \
  X(272, 34, 3) X(304, 38, 3) X(336, 42, 3) X(352, 44, 3) X(368, 46, 3) X(384, 48, 3) X(400, 50, 3) \
  X(416, 52, 3) X(432, 54, 3) X(448, 56, 3) X(464, 58, 3) X(480, 60, 3) X(496, 62, 3) X(512, 64, 3)
#define DCTS_SPLIT_TABLE_MORE(X) DCTS_SPLIT_TABLE_MORE_A(X) DCTS_SPLIT_TABLE_MORE_B(X)
#define DCTS_SPLIT_TABLE_BASE(X)                                                         \
  X(72, 18, 2) X(80, 20, 2) X(96, 24, 2) X(112, 28, 2) X(128, 32, 2) X(144, 36, 2) X(160, 40, 2)      \
  X(192, 24, 3) X(224, 28, 3) X(256, 32, 3) X(288, 36, 3) X(320, 40, 3)
#define DCTS_SPLIT_TABLE(X) DCTS_SPLIT_TABLE_BASE(X) DCTS_SPLIT_TABLE_MORE(X)
#endif
#endif

// tiles whose intermediate fits the register file of one CU: single fused launch X(N, M, L).
// (M, L) per edge is the fastest measured factorisation (e.g. 224: 28x8 roles 19 %, 14x16 roles 26 %;
// 128: 16x8 38 %, 32x4 35 %, 8x16 22 %; 288 = 18x16 spills at 128 VGPRs and loses to two launches)
#ifndef DCTS_FUSED_TABLE
#ifdef DCTS_DEV_FAST
#define DCTS_FUSED_TABLE(X) X(128, 16, 3) X(224, 14, 4)
#else
#define DCTS_FUSED_TABLE(X) \
  X(72, 9, 3) X(80, 10, 3) X(96, 12, 3) X(112, 14, 3) X(128, 16, 3) X(144, 18, 3) X(160, 10, 4) X(192, 12, 4) X(224, 14, 4) \
  X(256, 16, 4)
#endif
#endif

// two roles per wave X(N, M, L): tiles the 16-wave kernels cannot park (320 runs 48-column rounds
// so that its two LDS buffers fit the 160 KiB exactly, see Fused2Cfg)
#ifndef DCTS_FUSED2_TABLE
#define DCTS_FUSED2_TABLE(X) X(288, 18, 4) X(320, 20, 4)
#endif

// pipelined variant X(N, M, L)
#ifndef DCTS_PIPE_TABLE
#ifdef DCTS_DEV_FAST
#ifndef DCTS_DEV_M224
#define DCTS_DEV_M224 14
#define DCTS_DEV_L224 4
#endif
#define DCTS_PIPE_TABLE(X) X(128, 16, 3) X(224, DCTS_DEV_M224, DCTS_DEV_L224)
#else
// (measured against the fused kernel, % of 8 TB/s: 128: 49.2 vs 46.9, 224: 36.8 vs 33.1; it loses
// where the balanced dump pads much (72, 80, 144, 160) or spills (256), and ties at 112)
#define DCTS_PIPE_TABLE(X) X(128, 16, 3) X(224, 14, 4)
#endif
#endif
