// Driver of tests/test_id_decode.py::test_malformed_streams_*: a host program around the emulation build (FQSX_EMU: the id
// kernel as a 1-lane host "wave") and the host id decoder, built with -fsanitize=address where the compiler can, so that
// an access outside a buffer ends the run.  Reads a file of cases written by the test:
//   u32 n_cases, then per case: u8 header[17], u32 n_reads, u32 paired, u32 T, T x (u64 len, bytes)
// and sends every case through fqsx_id_decode_block and fqsx_idg_decode_block (a fresh codec each).  A call has to return
// an error, or lines that lie inside id_off's bounds.  Prints "DONE <errors> <decoded> <short>"; short = calls refused with
// FQSX_E_ARG (a worker with reads and a stream under 8 bytes).
#include "../../include/fqsx.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static bool inside(const uint8_t *ids, const uint64_t *off, uint32_t n) {
  if (!ids || !off || off[0] != 0) return false;
  uint64_t sum = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (off[i + 1] < off[i]) return false;
    for (uint64_t j = off[i]; j < off[i + 1]; ++j) sum += ids[j];   // (every byte is read: the sanitizer sees a line outside the buffer)
  }
  return sum + 1 != 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n_cases = 0;
  if (fread(&n_cases, 4, 1, f) != 1) return 2;
  long n_err = 0, n_ok = 0, n_short = 0;
  for (uint32_t c = 0; c < n_cases; ++c) {
    uint8_t header[17];
    uint32_t n_reads, paired, T;
    if (fread(header, 1, 17, f) != 17 || fread(&n_reads, 4, 1, f) != 1 || fread(&paired, 4, 1, f) != 1 || fread(&T, 4, 1, f) != 1) return 2;
    std::vector<std::vector<uint8_t>> st(T);
    std::vector<const uint8_t *> ptr(T);
    std::vector<uint64_t> len(T);
    for (uint32_t t = 0; t < T; ++t) {
      if (fread(&len[t], 8, 1, f) != 1) return 2;
      st[t].resize(len[t]);   // (exactly the stream's bytes: a read beyond them is a finding)
      if (len[t] && fread(st[t].data(), 1, len[t], f) != len[t]) return 2;
      ptr[t] = st[t].data();
    }
    for (int gpu = 0; gpu < 2; ++gpu) {
      const uint8_t *ids = nullptr;
      const uint64_t *off = nullptr;
      int rc;
      if (gpu) {
        fqsx_idg *q = nullptr;
        if (fqsx_idg_create(header, 0, &q)) return 3;
        rc = fqsx_idg_decode_block(q, ptr.data(), len.data(), n_reads, (int)paired, &ids, &off);
        if (!rc && !inside(ids, off, n_reads)) { printf("case %u: kernel output outside bounds\n", c); return 4; }
        fqsx_idg_destroy(q);
      } else {
        fqsx_id *q = nullptr;
        if (fqsx_id_create(header, &q)) return 3;
        rc = fqsx_id_decode_block(q, ptr.data(), len.data(), n_reads, (int)paired, &ids, &off);
        if (!rc && !inside(ids, off, n_reads)) { printf("case %u: host output outside bounds\n", c); return 4; }
        fqsx_id_destroy(q);
      }
      if (rc == FQSX_E_ARG) ++n_short; else if (rc) ++n_err; else ++n_ok;
    }
  }
  fclose(f);
  printf("DONE %ld %ld %ld\n", n_err, n_ok, n_short);
  return 0;
}
