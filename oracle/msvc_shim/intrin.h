// oracle/msvc_shim/intrin.h -- TEST INFRASTRUCTURE ONLY.
// The reference's tracers (och_h_octree.h, och_octree.cpp) include MSVC's
// <intrin.h> right after <immintrin.h> and read lanes of a __m128 through the
// members MSVC documents for that type (m128_f32, m128_u32).  This header is
// found in MSVC's place when oracle/Makefile builds _ref/ref_trace: it gives
// __m128 exactly those members and nothing else.  The wrapper converts from
// and to the compiler's own vector type, so every intrinsic the reference
// calls is the compiler's; no arithmetic is restated or replaced here.
#pragma once

#include <immintrin.h>
#include <cstdint>

struct och_msvc_m128
{
	union
	{
		__m128 v;
		float m128_f32[4];
		uint32_t m128_u32[4];
	};

	och_msvc_m128() = default;

	och_msvc_m128(__m128 x) : v(x) {}

	operator __m128() const { return v; }
};

#define __m128 och_msvc_m128
