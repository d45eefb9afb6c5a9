// Runs every table builder of smplpp_amd/csrc/model_tables.h on a model file and writes the tables out (tests/test_model_tables_cpu.py
// builds it with the address and undefined-behaviour sanitizers).  Host code only.
//   in : int64 V, F, has_scales | float W[V][24] | int64 kintree[24] | int32 faces[F][3] (1-based) | if has_scales: float P[V][3][207],
//        S[V][3][10], vt[V][3]
//   out: records { char name[16]; int64 element size, count; the elements }.  A refusal ends the file with a "refusal" record.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>

#include "../../smplpp_amd/csrc/model_tables.h"

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
static void put1(const char * name, T v)
{
  put(name, &v, 1);
}
static bool refused(const char * why)
{
  if(why) put("refusal", why, strlen(why));
  return why != nullptr;
}

template<class T>
static std::vector<T> get(FILE * f, size_t n)
{
  std::vector<T> v(n);
  if(n && fread(v.data(), sizeof(T), n, f) != n)
  {
    fprintf(stderr, "model_tables_dump: short read\n");
    exit(2);
  }
  return v;
}

static void run(int64_t V, int64_t F, const float * W, const int64_t * kintree, const int32_t * faces1, const float * P, const float * S,
                const float * vt)
{
  std::vector<int32_t> parent;
  if(refused(check_tree(kintree, parent)) || refused(check_faces(faces1, F, V))) return;
  const SkinWeights sw = skin_weights(W, V);
  put1<int32_t>("maxw", sw.maxw);
  {
    char forms[10];
    const char * envs[5] = {nullptr, "e", "h", "b", "v"};
    for(int i = 0; i < 5; i++) std::tie(forms[2 * i], forms[2 * i + 1]) = choose_forms(envs[i], sw.maxw, (V + 63) / 64);
    put("forms", forms, 10);
  }
  put("wIdx", sw.wIdx);
  put("wVal", sw.wVal);
  put("wSum", sw.wSum);
  if(P)
  {
    const HScales hs = h_scales(P, S, vt, V);
    if(refused(hs.refusal)) return;
    put1<float>("sB", hs.sB);
    put1<float>("sG", hs.sG);
  }
  const VertexGroups hg = h_vertex_groups(W, V);
  put("perm", hg.perm);
  put("flags", hg.flags);
  const JointLevels levels = joint_levels(parent);
  const ChainTables chain = chain_tables(parent, levels);
  put("depth", levels.depth);
  put1<int32_t>("nlev", levels.nlev);
  put1<int32_t>("chain_fast", chain.chain_fast ? 1 : 0);
  put("lvl", chain.lvl);
  const Adjacency adj = adjacency(faces1, F, V);
  put("faces", adj.faces);
  put("adjOff", adj.adjOff);
  put("adjFace", adj.adjFace);
  put("anc", ik_tree_tables(parent, levels));
  const RingTables ring = ik_ring_tables(adj.faces.data(), adj.adjOff.data(), adj.adjFace.data(), F, V);
  put1<int32_t>("madj", ring.madj);
  put("faceRing", ring.faceRing);
  put("faceMap", ring.faceMap);
}

int main(int argc, char ** argv)
{
  if(argc != 3)
  {
    fprintf(stderr, "usage: model_tables_dump MODEL TABLES\n");
    return 2;
  }
  FILE * f = fopen(argv[1], "rb");
  if(!f) return 2;
  const std::vector<int64_t> hdr = get<int64_t>(f, 3);
  const int64_t V = hdr[0], F = hdr[1];
  const std::vector<float> W = get<float>(f, (size_t)V * NJ);
  const std::vector<int64_t> kintree = get<int64_t>(f, NJ);
  const std::vector<int32_t> faces1 = get<int32_t>(f, (size_t)F * 3);
  std::vector<float> P, S, vt;
  if(hdr[2])
  {
    P = get<float>(f, (size_t)V * 3 * NP);
    S = get<float>(f, (size_t)V * 3 * NB);
    vt = get<float>(f, (size_t)V * 3);
  }
  fclose(f);
  g_out = fopen(argv[2], "wb");
  if(!g_out) return 2;
  run(V, F, W.data(), kintree.data(), faces1.data(), hdr[2] ? P.data() : nullptr, S.data(), vt.data());
  return fclose(g_out) == 0 ? 0 : 2;
}
