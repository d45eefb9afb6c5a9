// Runs the table builder of smplpp_amd/csrc/sequence_tables.h on a grouping file and writes the tables out (tests/test_sequence_cpu.py
// builds it with the address and undefined-behaviour sanitizers).  Host code only.
//   in : int64 P, shared_rows, has row_start, count | int64 row_start[count] (when has row_start; count = P + 1 for a sane P, else 0: the
//        builder must refuse such a P before it reads).  Without the flag row_start reaches the builder as NULL.
//   out: records { char name[16]; int64 element size, count; the elements }.  A refusal is the file's only record, "refusal".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../smplpp_amd/csrc/sequence_tables.h"

using namespace smplpp_hip;

static FILE * g_out;

template<class T>
static void put(const char * name, const T * data, size_t count)
{
  char nm[16] = {};
  strncpy(nm, name, 15);
  const int64_t es = sizeof(T), n = (int64_t)count;
  fwrite(nm, 1, 16, g_out);
  fwrite(&es, 8, 1, g_out);
  fwrite(&n, 8, 1, g_out);
  if(count) fwrite(data, sizeof(T), count, g_out);
}
template<class T>
static void put(const char * name, const std::vector<T> & v)
{
  put(name, v.data(), v.size());
}

static std::vector<int64_t> get(FILE * f, size_t n)
{
  std::vector<int64_t> v(n);
  if(n && fread(v.data(), 8, n, f) != n)
  {
    fprintf(stderr, "sequence_tables_dump: short read\n");
    exit(2);
  }
  return v;
}

int main(int argc, char ** argv)
{
  if(argc != 3)
  {
    fprintf(stderr, "usage: sequence_tables_dump GROUPS TABLES\n");
    return 2;
  }
  FILE * f = fopen(argv[1], "rb");
  if(!f) return 2;
  const std::vector<int64_t> hdr = get(f, 4);
  const std::vector<int64_t> row_start = get(f, hdr[2] ? (size_t)hdr[3] : 0);
  fclose(f);
  g_out = fopen(argv[2], "wb");
  if(!g_out) return 2;
  const SequenceTables t = sequence_tables(hdr[0], hdr[2] ? row_start.data() : nullptr, (int)hdr[1]);
  if(t.refusal) put("refusal", t.refusal, strlen(t.refusal));
  else
  {
    const int64_t dims[4] = {t.P, t.rows, t.frames, t.shared_rows};
    put("dims", dims, 4);
    put("row_start", t.row_start);
    put("frame_start", t.frame_start);
    put("problem_of", t.problem_of);
    put("row_of", t.row_of);
    put("frame_of", t.frame_of);
  }
  return fclose(g_out) == 0 ? 0 : 2;
}
