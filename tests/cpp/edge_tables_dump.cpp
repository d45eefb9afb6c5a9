// Runs the edge-table builder and the plan functions of smplpp_amd/csrc/edge_tables.h and writes the results out
// (tests/test_self_contact_cpu.py builds it with the address and undefined-behaviour sanitizers).  Host code only.
//   edge_tables_dump FACES TABLES
//     in : int64 V, F | int32 faces[3 F], 0-based
//     out: records { char name[16]; int64 element size, count; the elements }.  A refusal is the file's only record, "refusal".
//   edge_tables_dump --plan V...
//     prints one line per V: V lds_bytes opt_in max_sweeps mask_words refused(0|1)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../smplpp_amd/csrc/edge_tables.h"

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

int main(int argc, char ** argv)
{
  if(argc >= 2 && !strcmp(argv[1], "--plan"))
  {
    for(int i = 2; i < argc; i++)
    {
      const int64_t V = atoll(argv[i]);
      const GeodesicPlan p = geodesic_plan(V);
      printf("%lld %lld %d %lld %lld %d\n", (long long)V, (long long)p.lds_bytes, p.opt_in ? 1 : 0, (long long)p.max_sweeps,
             (long long)contact_mask_words(V), p.refusal ? 1 : 0);
    }
    return 0;
  }
  if(argc != 3)
  {
    fprintf(stderr, "usage: edge_tables_dump FACES TABLES | --plan V...\n");
    return 2;
  }
  FILE * f = fopen(argv[1], "rb");
  if(!f) return 2;
  int64_t hdr[2];
  if(fread(hdr, sizeof(int64_t), 2, f) != 2) return 2;
  // (an exact-size heap array: a read past its end is a sanitizer report)
  std::vector<int32_t> faces(hdr[1] > 0 ? (size_t)hdr[1] * 3 : 0);
  if(!faces.empty() && fread(faces.data(), sizeof(int32_t), faces.size(), f) != faces.size())
  {
    fprintf(stderr, "edge_tables_dump: short read\n");
    return 2;
  }
  fclose(f);
  g_out = fopen(argv[2], "wb");
  if(!g_out) return 2;
  const EdgeTable t = edge_table(hdr[0], hdr[1], faces.empty() ? nullptr : faces.data());
  if(t.refusal) put("refusal", t.refusal, strlen(t.refusal));
  else
  {
    const int64_t dims[2] = {t.V, t.nnz};
    put("dims", dims, 2);
    put("off", t.off);
    put("adj", t.adj);
    put("src", t.src);
  }
  return fclose(g_out) == 0 ? 0 : 2;
}
