// Runs the table builder of smplpp_amd/csrc/measure_tables.h on a regions file and writes the tables out (tests/test_measure_cpu.py
// builds it with the address and undefined-behaviour sanitizers).  Host code only.
//   in : int64 F, R, S, rows, entries | int64 region_ptr[rows] | int64 region_face[entries] | int64 section_region[max(S, 0)]
//        (rows = R + 1 for a well-formed file; a refusal case may claim an R or an S its arrays do not hold: the builder must refuse
//        before it reads them)
//   out: records { char name[16]; int64 element size, count; the elements }.  A refusal is the file's only record, "refusal".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../smplpp_amd/csrc/measure_tables.h"

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
  if(n && fread(v.data(), sizeof(int64_t), n, f) != n)
  {
    fprintf(stderr, "measure_tables_dump: short read\n");
    exit(2);
  }
  return v;
}

int main(int argc, char ** argv)
{
  if(argc != 3)
  {
    fprintf(stderr, "usage: measure_tables_dump REGIONS TABLES\n");
    return 2;
  }
  FILE * f = fopen(argv[1], "rb");
  if(!f) return 2;
  const std::vector<int64_t> hdr = get(f, 5);
  const std::vector<int64_t> ptr = get(f, (size_t)hdr[3]);
  const std::vector<int64_t> face = get(f, (size_t)hdr[4]);
  const std::vector<int64_t> sec = get(f, hdr[2] > 0 ? (size_t)hdr[2] : 0);
  fclose(f);
  g_out = fopen(argv[2], "wb");
  if(!g_out) return 2;
  // (exact-size heap arrays: a read past the end of any of them is a sanitizer report)
  const MeasureTables t = measure_tables(hdr[0], hdr[1], ptr.empty() ? nullptr : ptr.data(), face.empty() ? nullptr : face.data(), hdr[2],
                                         sec.empty() ? nullptr : sec.data());
  if(t.refusal) put("refusal", t.refusal, strlen(t.refusal));
  else
  {
    const int64_t dims[4] = {t.R, t.nnz, t.S, t.F};
    put("dims", dims, 4);
    put("regionPtr", t.regionPtr);
    put("regionFace", t.regionFace);
    put("facePtr", t.facePtr);
    put("faceRegion", t.faceRegion);
    put("faceSlot", t.faceSlot);
    put("secPtr", t.secPtr);
    put("secId", t.secId);
    put("secRegion", t.secRegion);
  }
  return fclose(g_out) == 0 ? 0 : 2;
}
