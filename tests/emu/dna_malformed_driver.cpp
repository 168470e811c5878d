// Driver of tests/test_dna_malformed.py: a host program around the emulation build (FQSX_EMU: the DNA decode kernels as a
// 1-lane host "wave") and the CPU oracle (oracle/fqs_oracle.cpp), built with -fsanitize=address where the compiler can, so
// that an access outside a buffer ends the run.  Reads a file of cases written by the test:
//   u32 n_groups, then per group:
//     u8 header[17], u32 tiny (1: table sizes of 64 slots at 85 % load through the environment), u32 n_good
//     n_good x block: u32 n_reads, u64 off[n_reads + 1], u8 bases[off[n_reads]], T x (u64 len, bytes)     (T = header[4])
//     u32 n_cases, then per case: u32 kind, u32 n_reads, u64 off[n_reads + 1], T x (u64 len, bytes)
// A case is the group's last good block in a damaged version; kind 0: damaged streams, 1: damaged offsets with the streams
// intact, 2: offsets the entry point has to refuse (FQSX_E_ARG).  For every case a fresh codec decodes the leading good blocks
// (they must come back as given) and then the damaged one, into a buffer of exactly off[n_reads] bytes and from stream buffers of
// exactly their bytes.  Required of every call: it returns; with a code, or with every output byte one of ACGTN.  After an error
// the codec is destroyed and a fresh one decodes the undamaged blocks.  Kind 0 also goes through the oracle behind the same
// good blocks: both decoders fail or both give the same bases, and then the decoder's tables (distinct s-mers, b-mers, pairs,
// contexts) are those of an emulation encoder that encodes these bases as the last block behind the same good blocks.
// Prints "CASE <group> <case> mode <m> kind <k>: <code> <error text>" per case, "SPLIT <dna_mode> <errors> <decoded>" per mode over the kind-0 cases, "TEXT <message>" with the first decode error's
// text, and "DONE <cases>".  Exit code 0: all of it held.
#include "../../include/fqsx.h"
#include "../../oracle/fqs_oracle.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

struct Block {
  uint32_t n = 0;
  std::vector<uint64_t> off;
  std::vector<uint8_t> bases;              // good blocks only
  std::vector<uint8_t *> st;               // every stream in an allocation of exactly its bytes
  std::vector<uint64_t> len;
  ~Block() { for (uint8_t *p : st) free(p); }
};

bool get(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

bool read_block(FILE *f, uint32_t T, bool with_bases, Block &b) {
  if (!get(f, &b.n, 4)) return false;
  b.off.resize((size_t)b.n + 1);
  if (!get(f, b.off.data(), b.off.size() * 8)) return false;
  if (with_bases) {
    b.bases.resize(b.off[b.n]);
    if (!get(f, b.bases.data(), b.bases.size())) return false;
  }
  b.st.assign(T, nullptr);
  b.len.assign(T, 0);
  for (uint32_t t = 0; t < T; ++t) {
    if (!get(f, &b.len[t], 8)) return false;
    b.st[t] = (uint8_t *)malloc(b.len[t]);   // (exactly the stream's bytes: a read beyond them is a finding)
    if (!get(f, b.st[t], b.len[t])) return false;
  }
  return true;
}

int fail(uint32_t g, uint32_t c, const char *what) {
  printf("group %u case %u: %s (%s)\n", g, c, what, fqsx_last_error());
  return 4;
}

bool all_bases(const uint8_t *p, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (p[i] != 'A' && p[i] != 'C' && p[i] != 'G' && p[i] != 'T' && p[i] != 'N') return false;
  return true;
}

// the good blocks [0, n) through codec q; each has to come back as given
bool decode_good(fqsx_dna *q, const std::vector<Block> &good, size_t n) {
  for (size_t g = 0; g < n; ++g) {
    const Block &b = good[g];
    std::vector<uint8_t> out(b.bases.size() + 1, '#');
    if (fqsx_dna_decode_block(q, b.st.data(), b.len.data(), b.off.data(), b.n, (uint32_t)g, out.data())) return false;
    if (memcmp(out.data(), b.bases.data(), b.bases.size()) != 0 || out[b.bases.size()] != '#') return false;
  }
  return true;
}

const int CAP_KEYS[4] = {0, 1, 10, 6};   // fqsx_dna_capacity: distinct s-mers, b-mers, pairs, contexts

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n_groups = 0;
  if (!get(f, &n_groups, 4)) return 2;
  long split[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}}, n_cases_all = 0;
  bool text_shown = false;
  for (uint32_t g = 0; g < n_groups; ++g) {
    uint8_t header[17];
    uint32_t tiny = 0, n_good = 0, n_cases = 0;
    if (!get(f, header, 17) || !get(f, &tiny, 4) || !get(f, &n_good, 4) || n_good == 0) return 2;
    const uint32_t T = header[4], mode = header[5];
    if (mode > 3) return 2;
    if (tiny) {
      setenv("FQSX_GTAB_INIT", "64", 1); setenv("FQSX_TAB_LOAD_PCT", "85", 1);
      if (mode >= 2) setenv("FQSX_PTAB_INIT", "64", 1); else unsetenv("FQSX_PTAB_INIT");
    } else {
      unsetenv("FQSX_GTAB_INIT"); unsetenv("FQSX_TAB_LOAD_PCT"); unsetenv("FQSX_PTAB_INIT");
    }
    std::vector<Block> good(n_good);
    for (Block &b : good)
      if (!read_block(f, T, true, b)) return 2;
    const uint32_t gen = n_good - 1;
    if (!get(f, &n_cases, 4)) return 2;
    for (uint32_t c = 0; c < n_cases; ++c, ++n_cases_all) {
      uint32_t kind = 0;
      Block bad;
      if (!get(f, &kind, 4) || !read_block(f, T, false, bad)) return 2;
      const uint64_t n_out = bad.off[bad.n];
      // ---- the decoder under test
      fqsx_dna *dec = nullptr;
      if (fqsx_dna_create(header, 0, &dec)) return fail(g, c, "create");
      if (!decode_good(dec, good, gen)) return fail(g, c, "a leading good block did not decode to its input");
      uint8_t *out = (uint8_t *)malloc(n_out);   // (exactly off[n_reads] bytes)
      if (n_out) memset(out, '#', n_out);
      const int rc = fqsx_dna_decode_block(dec, bad.st.data(), bad.len.data(), bad.off.data(), bad.n, gen, out);
      const std::string text = fqsx_last_error();
      printf("CASE %u %u mode %u kind %u: %d %s\n", g, c, mode, kind, rc, rc ? text.c_str() : "");
      if (kind == 2 && rc != FQSX_E_ARG) return fail(g, c, "offsets that descend / an odd paired count were not refused with FQSX_E_ARG");
      if (kind != 2 && rc == FQSX_E_ARG) return fail(g, c, "FQSX_E_ARG for a block whose arguments are in order");
      if (!rc && !all_bases(out, n_out)) return fail(g, c, "code 0, but an output byte is not one of ACGTN");
      if (rc == FQSX_E_DEVICE) {   // the text names the decoder
        if (text.find("decod") == std::string::npos || text.find("encode") != std::string::npos) return fail(g, c, "a decode error's text does not name the decoder");
        if (!text_shown && text.find("in decode kernel") != std::string::npos) { printf("TEXT %s\n", text.c_str()); text_shown = true; }
      }
      uint64_t cap_dec[16] = {0};
      if (!rc && fqsx_dna_capacity(dec, cap_dec)) return fail(g, c, "capacity");
      fqsx_dna_destroy(dec);   // (after an error too: it has to complete)
      if (rc) {                // ... and a fresh codec decodes the undamaged blocks
        fqsx_dna *again = nullptr;
        if (fqsx_dna_create(header, 0, &again)) return fail(g, c, "create");
        if (!decode_good(again, good, n_good)) return fail(g, c, "after an error: a fresh codec did not decode the undamaged blocks");
        fqsx_dna_destroy(again);
      }
      if (kind == 0) {
        split[mode][rc ? 0 : 1] += 1;
        // ---- the oracle behind the same good blocks
        fqo_codec *o = fqo_create(header);
        if (!o) return fail(g, c, "oracle create");
        for (uint32_t b = 0; b < gen; ++b) {
          std::vector<uint8_t> tmp(good[b].bases.size() + 1);
          if (fqo_decode_block(o, good[b].st.data(), good[b].len.data(), good[b].off.data(), good[b].n, b, tmp.data()) ||
              memcmp(tmp.data(), good[b].bases.data(), good[b].bases.size()) != 0)
            return fail(g, c, "oracle: a leading good block did not decode to its input");
        }
        uint8_t *oout = (uint8_t *)malloc(n_out);
        if (n_out) memset(oout, '#', n_out);
        const int orc = fqo_decode_block(o, bad.st.data(), bad.len.data(), bad.off.data(), bad.n, gen, oout);
        fqo_destroy(o);
        if ((rc != 0) != (orc != 0)) { printf("decoder %d, oracle %d: ", rc, orc); return fail(g, c, "one decoder fails where the other gives bases"); }
        if (!rc && memcmp(out, oout, n_out) != 0) return fail(g, c, "decoder and oracle give different bases");
        free(oout);
        if (!rc) {   // what the decoder learnt = what an encoder learns from these bases
          fqsx_dna *enc = nullptr;
          if (fqsx_dna_create(header, 0, &enc)) return fail(g, c, "create");
          std::vector<const uint8_t *> st(T);
          std::vector<uint64_t> ln(T);
          for (uint32_t b = 0; b < gen; ++b)
            if (fqsx_dna_encode_block(enc, good[b].bases.data(), good[b].off.data(), good[b].n, b, st.data(), ln.data())) return fail(g, c, "encode of a good block");
          std::vector<uint8_t> in(out, out + n_out);
          in.push_back('A');   // (a block of 0 bases still has a pointer)
          if (fqsx_dna_encode_block(enc, in.data(), bad.off.data(), bad.n, gen, st.data(), ln.data())) return fail(g, c, "encode of the decoded bases");
          uint64_t cap_enc[16] = {0};
          if (fqsx_dna_capacity(enc, cap_enc)) return fail(g, c, "capacity");
          fqsx_dna_destroy(enc);
          for (int k : CAP_KEYS)
            if (cap_dec[k] != cap_enc[k]) {
              printf("capacity[%d]: decoder %llu, encoder %llu: ", k, (unsigned long long)cap_dec[k], (unsigned long long)cap_enc[k]);
              return fail(g, c, "the decoder's tables differ from those of an encoder of the bases it returned");
            }
        }
      }
      free(out);
    }
  }
  fclose(f);
  for (int m = 0; m < 4; ++m) printf("SPLIT %d %ld %ld\n", m, split[m][0], split[m][1]);
  printf("DONE %ld\n", n_cases_all);
  return 0;
}
