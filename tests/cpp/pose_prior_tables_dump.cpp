// Runs the table builder of smplpp_amd/csrc/pose_prior_tables.h on a prior file and writes the tables out (tests/test_pose_prior_cpu.py
// builds it with the address and undefined-behaviour sanitizers).  Host code only.
//   in : int64 M, D, has mixture arrays, has lo, has hi, has weight | float mean[M D], mat[M D D], offset[M] (when has mixture arrays) |
//        float lo[D] | hi[D] | weight[D] (each when its flag is set).  An array whose flag is 0 reaches the builder as NULL.  A refusal
//        case may claim an M or a D its arrays do not hold: the file then carries no arrays and the builder must refuse before it reads.
//   out: records { char name[16]; int64 element size, count; the elements }.  A refusal is the file's only record, "refusal".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../smplpp_amd/csrc/pose_prior_tables.h"

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
static void put(const char * name, const std::vector<float> & v)
{
  put(name, v.data(), v.size());
}

template<class T>
static std::vector<T> get(FILE * f, size_t n)
{
  std::vector<T> v(n);
  if(n && fread(v.data(), sizeof(T), n, f) != n)
  {
    fprintf(stderr, "pose_prior_tables_dump: short read\n");
    exit(2);
  }
  return v;
}

int main(int argc, char ** argv)
{
  if(argc != 3)
  {
    fprintf(stderr, "usage: pose_prior_tables_dump PRIOR TABLES\n");
    return 2;
  }
  FILE * f = fopen(argv[1], "rb");
  if(!f) return 2;
  const std::vector<int64_t> hdr = get<int64_t>(f, 6);
  const int64_t M = hdr[0], D = hdr[1];
  const bool sane = M >= 0 && M <= PRIOR_MAX_M && D >= 1 && D <= PRIOR_MAX_D; // (else the file carries no arrays)
  const bool mix = sane && hdr[2];
  const std::vector<float> mean = get<float>(f, mix ? (size_t)(M * D) : 0), mat = get<float>(f, mix ? (size_t)(M * D * D) : 0),
                           offset = get<float>(f, mix ? (size_t)M : 0);
  const std::vector<float> lo = get<float>(f, sane && hdr[3] ? (size_t)D : 0), hi = get<float>(f, sane && hdr[4] ? (size_t)D : 0),
                           weight = get<float>(f, sane && hdr[5] ? (size_t)D : 0);
  fclose(f);
  g_out = fopen(argv[2], "wb");
  if(!g_out) return 2;
  // (an empty vector's data() may be non-null: the flags decide)
  const PosePriorTables t = pose_prior_tables(M, D, hdr[2] ? mean.data() : nullptr, hdr[2] ? mat.data() : nullptr, hdr[2] ? offset.data() : nullptr,
                                              hdr[3] ? lo.data() : nullptr, hdr[4] ? hi.data() : nullptr, hdr[5] ? weight.data() : nullptr);
  if(t.refusal) put("refusal", t.refusal, strlen(t.refusal));
  else
  {
    const int64_t dims[3] = {t.M, t.D, t.limits ? 1 : 0};
    put("dims", dims, 3);
    put("mean", t.mean);
    put("mat", t.mat);
    put("matT", t.matT);
    put("offset", t.offset);
    put("lo", t.lo);
    put("hi", t.hi);
    put("weight", t.weight);
  }
  return fclose(g_out) == 0 ? 0 : 2;
}
