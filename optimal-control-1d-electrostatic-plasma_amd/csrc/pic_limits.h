// pic_limits.h -- the launch constants that the kernels and the launch planner (host_plan.h) share.  No HIP in here: the planner
// compiles with a plain host compiler.  The kernels' static_asserts tie their static __shared__ arrays to the two LDS figures.
#pragma once
#include <cstddef>

constexpr int kMaxFeedbackModes = 16;
constexpr int BLOCK = 512;          // sweep workgroup: 8 waves of 64 (512 beat 256 by 2.7 % and 128 by 11 % at config 2)
constexpr int WAVES = BLOCK / 64;
constexpr size_t kSweepStaticLds = (2 * WAVES + 2) * sizeof(double);     // sweep_kernel's static __shared__ arrays
constexpr size_t kResidentStaticLds = (4 * 8 + 4 + 2 * kMaxFeedbackModes) * sizeof(double);   // resident_kernel's static __shared__ arrays (NW = 8)
// a workgroup may use 64 KB of LDS: the dynamic part the planner sizes plus the kernels' static arrays
constexpr size_t kLdsLimit = 64 * 1024;
