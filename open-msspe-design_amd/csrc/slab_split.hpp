// slab_split.hpp -- how a slab of a thal-scored site pass is cut when its matches overran the work list.  Plain
// integer arithmetic (C++17, no HIP): capi.cpp run_slabs executes the rule, and msspe_host_slab_split hands it to the
// CPU tests (tests/test_slab_split_model.py) as it stands.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace msspe {

// Outer range [o0, o1) -- runs of the background pass, segment groups of the coverage passes -- x primers [p0, p1).
struct Slab { long o0, o1; int p0, p1; };

// The parts of a slab that listed `count` > cap matches, appended to `out` in ascending order: as many as the count
// says, by the outer axis while it has several elements, then by primers.  false, nothing appended: one outer element
// against one primer cannot be cut.
inline bool split_slab(const Slab &s, uint64_t count, uint64_t cap, std::vector<Slab> &out)
{
    const uint64_t outer = (uint64_t)(s.o1 - s.o0), prim = (uint64_t)(s.p1 - s.p0);
    const uint64_t want = (2 * count + cap - 1) / cap;   // parts that would be half full at this density
    if (outer > 1) {
        const uint64_t parts = std::min(outer, want);
        for (uint64_t q = 0; q < parts; ++q)
            out.push_back({s.o0 + (long)(outer * q / parts), s.o0 + (long)(outer * (q + 1) / parts), s.p0, s.p1});
    } else if (prim > 1) {
        const uint64_t parts = std::min(prim, want);
        for (uint64_t q = 0; q < parts; ++q)
            out.push_back({s.o0, s.o1, s.p0 + (int)(prim * q / parts), s.p0 + (int)(prim * (q + 1) / parts)});
    }
    return outer > 1 || prim > 1;
}

}  // namespace msspe
