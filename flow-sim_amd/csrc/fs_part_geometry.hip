// kernel instantiations of libflowsim_hip.so, part "geometry": the members' polylines, bed levels, roughnesses and stage tables of a
// geometry ensemble built on the device (fs_member_geo.hpp).  These kernels are not step kernels: they have no row in
// fs_entry_list.hpp and no entry in the dispatch table.
//
// The whole translation unit is compiled without contraction: the stage tables it writes are held to the host builder's
// (fs_stage_table.hpp: build_stage_table) bit for bit, and that one rounds every product before it adds.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "fs_member_geo.hpp"

namespace fs {
namespace {

dim3 member_grid(const MemberGeoArgs &a) { return dim3((unsigned)(a.B * ((a.N + kMemberLanes - 1) / kMemberLanes))); }

}  // namespace

bool launch_member_sections(const MemberGeoArgs &a, hipStream_t st) {
  hipLaunchKernelGGL((member_sections_kernel<kMemberLanes>), member_grid(a), dim3(kMemberLanes), 0, st, a);
  return true;
}

bool launch_member_tables(const MemberGeoArgs &a, hipStream_t st) {
  hipLaunchKernelGGL((member_tables_kernel<kMemberLanes>), member_grid(a), dim3(kMemberLanes), 0, st, a);
  return true;
}

}  // namespace fs
