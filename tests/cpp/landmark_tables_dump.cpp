// Runs the table builder of smplpp_amd/csrc/landmark_tables.h on a regressor file and writes the tables out (tests/test_keypoints_cpu.py
// builds it with the address and undefined-behaviour sanitizers).  Host code only.
//   in : int64 L, S, rows, entries | int64 row_ptr[rows] | int64 col[entries] | float val[entries]   (rows = L + 1 for a well-formed
//        file; a refusal case may claim an L or an nnz its arrays do not hold: the builder must refuse before it reads them)
//   out: records { char name[16]; int64 element size, count; the elements }.  A refusal is the file's only record, "refusal".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../smplpp_amd/csrc/landmark_tables.h"

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

template<class T>
static std::vector<T> get(FILE * f, size_t n)
{
  std::vector<T> v(n);
  if(n && fread(v.data(), sizeof(T), n, f) != n)
  {
    fprintf(stderr, "landmark_tables_dump: short read\n");
    exit(2);
  }
  return v;
}

int main(int argc, char ** argv)
{
  if(argc != 3)
  {
    fprintf(stderr, "usage: landmark_tables_dump REGRESSOR TABLES\n");
    return 2;
  }
  FILE * f = fopen(argv[1], "rb");
  if(!f) return 2;
  const std::vector<int64_t> hdr = get<int64_t>(f, 4);
  const std::vector<int64_t> row_ptr = get<int64_t>(f, (size_t)hdr[2]);
  const std::vector<int64_t> col = get<int64_t>(f, (size_t)hdr[3]);
  const std::vector<float> val = get<float>(f, (size_t)hdr[3]);
  fclose(f);
  g_out = fopen(argv[2], "wb");
  if(!g_out) return 2;
  const LandmarkTables t = landmark_tables(hdr[0], hdr[1], row_ptr.data(), col.data(), val.data());
  if(t.refusal) put("refusal", t.refusal, strlen(t.refusal));
  else
  {
    const int64_t dims[3] = {t.L, t.nnz, t.S};
    put("dims", dims, 3);
    put("rowPtr", t.rowPtr);
    put("col", t.col);
    put("val", t.val);
    put("srcPtr", t.srcPtr);
    put("srcRow", t.srcRow);
    put("srcVal", t.srcVal);
  }
  return fclose(g_out) == 0 ? 0 : 2;
}
