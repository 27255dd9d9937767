// kernel instantiations of libflowsim_hip.so, part "nodiag" (see fs_entry_list.hpp)
#include "fs_entries.hpp"

FS_LIST_NODIAG(FS_INSTANTIATE)
FS_LIST_TAIL(FS_INSTANTIATE)
