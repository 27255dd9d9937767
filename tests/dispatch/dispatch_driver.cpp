// dispatch_driver.cpp - the kernel dispatch of libflowsim_hip.so (fs_dispatch.hpp) over the key table built from the library's own
// lists (fs_entry_list.hpp), under the system compiler and its sanitizers (tests/test_dispatch.py):
//   dispatch_driver table                    the table: one line of ten numbers per entry, in the order of fs::KernelKey
//   dispatch_driver grid OUT                 the chosen index (or -1) of every query of the grid, int16, to the file OUT
//   dispatch_driver query dtype sec N usk dsk need_diag need_any hetero
//                                            the chosen index and, on the next line, the reason where there is none
//   dispatch_driver plan IN                  IN: one launch per line: entry sec N B n_steps storage_downstream.  Prints per line whether
//                                            the entry fits a batch of its own kind with N nodes, then fs::plan_launch: passes,
//                                            kc_scratch_elems, team_size, team_mail_bytes, keep_entry, keep_stage, and the bytes of one
//                                            mailbox as the team kernel strides them (fs::team_mailbox_bytes)
// The overrides come from the environment, as in the library (FS_KERNEL_INDEX, FS_KERNEL_SHAPE, FS_KERNEL_GENERAL, FS_NO_TEAM, FS_TEAM_M).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fs_entry_list.hpp"
#include "fs_dispatch.hpp"

struct Row { fs::KernelKey key; };
#define ROW(...) {FS_KEY(__VA_ARGS__)},
static const Row kKeys[] = {FS_ACTIVE_LIST(ROW)};
static const int kNumKeys = (int)(sizeof(kKeys) / sizeof(kKeys[0]));

// the grid, outermost first: dtype, section mode, N, upstream kind, downstream kind, need_diag, need_any, hetero
static const int kGridN[] = {2, 64, 65, 121, 128, 129, 256, 512, 513, 1024, 2048, 4096, 4097, 8192, 9000, 16384, 16385, 32768, 32769};

int main(int argc, char **argv) {
  const fs::Overrides o = fs::overrides_from_environment();
  if (argc == 2 && !std::strcmp(argv[1], "table")) {
    for (const Row &r : kKeys) {
      const fs::KernelKey &k = r.key;
      std::printf("%d %d %d %d %d %d %d %d %d %d\n", k.dtype, k.sec, k.M, k.W, k.full, k.bck, k.diag, k.longk, k.tail, k.team);
    }
    return 0;
  }
  if (argc == 3 && !std::strcmp(argv[1], "grid")) {
    std::vector<int16_t> out;
    fs::Query q;
    for (q.dtype = FS_F64; q.dtype <= FS_F32; ++q.dtype)
      for (q.sec = FS_SEC_RECT_UNIFORM; q.sec <= FS_SEC_IRREGULAR; ++q.sec)
        for (int N : kGridN)
          for (q.usk = 0; q.usk <= FS_BC_HOST_ROW; ++q.usk)
            for (q.dsk = 0; q.dsk <= FS_BC_HOST_ROW; ++q.dsk)
              for (int need_diag = 0; need_diag < 2; ++need_diag)
                for (int need_any = 0; need_any < 2; ++need_any)
                  for (q.hetero = 0; q.hetero < 4; ++q.hetero) {
                    q.N = N; q.need_diag = need_diag != 0; q.need_any = need_any != 0;
                    out.push_back((int16_t)fs::pick(kKeys, kNumKeys, q, o, nullptr));
                  }
    FILE *f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), sizeof(int16_t), out.size(), f) != out.size() || std::fclose(f) != 0) return 2;
    return 0;
  }
  if (argc == 10 && !std::strcmp(argv[1], "query")) {
    int v[8];
    for (int i = 0; i < 8; ++i) v[i] = std::atoi(argv[2 + i]);
    fs::Query q;
    q.dtype = v[0]; q.sec = v[1]; q.N = v[2]; q.usk = v[3]; q.dsk = v[4]; q.need_diag = v[5] != 0; q.need_any = v[6] != 0; q.hetero = v[7];
    std::string why;
    const int chosen = fs::pick(kKeys, kNumKeys, q, o, &why);
    std::printf("%d\n%s\n", chosen, why.c_str());
    return 0;
  }
  if (argc == 3 && !std::strcmp(argv[1], "plan")) {
    FILE *f = std::fopen(argv[2], "r");
    if (!f) return 2;
    int entry, sec, n_steps, storage;
    long long B, N;
    while (std::fscanf(f, "%d %d %lld %lld %d %d", &entry, &sec, &N, &B, &n_steps, &storage) == 6) {
      if (entry < 0 || entry >= kNumKeys) return 2;
      const fs::KernelKey &k = kKeys[entry].key;
      fs::Query q;      // a batch the entry was compiled for: its type, mode and boundary pair (any pair: flow in, normal depth out)
      q.dtype = k.dtype; q.sec = k.sec; q.N = (int)N; q.usk = FS_BC_FLOW_HYDROGRAPH; q.dsk = k.bck >= 2 ? k.bck - 2 : FS_BC_NORMAL_DEPTH;
      q.need_diag = k.diag != 0;
      const fs::LaunchPlan p = fs::plan_launch(k, sec, (size_t)B, (size_t)N, n_steps, storage != 0);
      std::printf("%d %d %zu %d %zu %d %d %zu\n", fs::fits(k, q, o) ? 1 : 0, p.passes, p.kc_scratch_elems, p.team_size, p.team_mail_bytes,
                  p.keep_entry ? 1 : 0, p.keep_stage ? 1 : 0, fs::team_mailbox_bytes(p.team_size, k.W));
    }
    std::fclose(f);
    return 0;
  }
  std::fprintf(stderr, "usage: %s table | grid OUT | query dtype sec N usk dsk need_diag need_any hetero | plan IN\n", argv[0]);
  return 1;
}
