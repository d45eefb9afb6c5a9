// smplpp::cloudKnn / cloudNormals / cloudFarthestPoints over the C ABI — header-only C++ shim of the scan preparation (smplpp_cloud_knn,
// smplpp_cloud_normals, smplpp_cloud_farthest_points): the k nearest cloud points of every query in the order (distance, index), a normal
// and a surface variation per point from those lists, and a thinning of a cloud to M well-spread points.  What a raw scan needs before
// pointMeshDistanceCompatible / meshPointDistanceCompatible take it.  No reference counterpart: the reference never fits to a cloud.
#ifndef SMPLPP_SHIM_CLOUD_H
#define SMPLPP_SHIM_CLOUD_H

#include <limits>

#include "SMPL.h"

namespace smplpp
{
namespace detail
{
struct CloudShape
{
  int64_t n, K;
};
inline CloudShape cloudShape(const Tensor & points, const char * what)
{
  if(points.dtype != kFloat32 || points.dim() != 3 || points.size(2) != 3) throw Exception("Cloud", what);
  return CloudShape{points.size(0), points.size(1)};
}
inline Tensor cloudInts(const std::vector<int32_t> & v, std::vector<int64_t> shape)
{
  Tensor t(std::move(shape), kInt64);
  t.idata.assign(v.begin(), v.end());
  return t;
}
} // namespace detail

// index [N,Q,k] kInt64 and sqdist [N,Q,k], ordered by (squared distance, index); count [N,Q] kInt64; ranks from count on hold (-1, 0)
struct CloudNeighbours
{
  Tensor index, sqdist, count;
};
// The k (1..32) nearest of points [N,K,3] for every query of queries [N,Q,3]; an undefined `queries`: the cloud queries itself, and a
// point is not its own neighbour.  Only points within maxDist are listed (infinity: no cap).
inline CloudNeighbours cloudKnn(const Tensor & points, int k, const Tensor & queries = Tensor(),
                                float maxDist = std::numeric_limits<float>::infinity(), int device = 0)
{
  const char * what = "Cannot search the cloud!";
  const detail::CloudShape s = detail::cloudShape(points, what);
  int64_t Q = s.K;
  if(queries.defined())
  {
    if(detail::cloudShape(queries, what).n != s.n) throw Exception("Cloud", what);
    Q = queries.size(1);
  }
  if(k < 1 || k > 32 || !(maxDist >= 0.0f)) throw Exception("Cloud", what);
  std::vector<int32_t> index((size_t)(s.n * Q * k)), count((size_t)(s.n * Q));
  CloudNeighbours r{Tensor(), Tensor({s.n, Q, (int64_t)k}), Tensor()};
  check(smplpp_cloud_knn(device, s.n, s.K, points.ptr(), Q, queries.defined() ? queries.ptr() : nullptr, k, maxDist * maxDist, index.data(),
                         r.sqdist.ptr(), count.data(), SMPLPP_HOST, nullptr),
        "Cloud");
  r.index = detail::cloudInts(index, {s.n, Q, (int64_t)k});
  r.count = detail::cloudInts(count, {s.n, Q});
  return r;
}

// normal [N,K,3], curvature [N,K] (the surface variation l0 / (l0 + l1 + l2)), status [N,K] kInt64 (1: fewer than two usable neighbours,
// the normal is zero; 2: the normal is not unique)
struct CloudNormals
{
  Tensor normal, curvature, status;
};
// From the neighbour lists index [N,K,k] of cloudKnn in self-query mode.  viewpoint [3] or [N,3]: the normals point towards it;
// undefined: the component of largest magnitude is positive.
inline CloudNormals cloudNormals(const Tensor & points, const Tensor & index, const Tensor & viewpoint = Tensor(), float minGap = 0.0f,
                                 int device = 0)
{
  const char * what = "Cannot estimate the normals!";
  const detail::CloudShape s = detail::cloudShape(points, what);
  if((index.dtype != kInt64 && index.dtype != kInt32) || index.dim() != 3 || index.size(0) != s.n || index.size(1) != s.K || index.size(2) < 1)
    throw Exception("Cloud", what);
  int64_t Vn = 0;
  if(viewpoint.defined())
  {
    if(viewpoint.dtype != kFloat32 || (viewpoint.numel() != 3 && viewpoint.numel() != 3 * s.n)) throw Exception("Cloud", what);
    Vn = viewpoint.numel() / 3;
  }
  std::vector<int32_t> status((size_t)(s.n * s.K));
  CloudNormals r{Tensor({s.n, s.K, 3}), Tensor({s.n, s.K}), Tensor()};
  check(smplpp_cloud_normals(device, s.n, s.K, points.ptr(), (int)index.size(2), index.data_ptr<int32_t>(), Vn ? viewpoint.ptr() : nullptr, Vn,
                             minGap, r.normal.ptr(), r.curvature.ptr(), status.data(), SMPLPP_HOST, nullptr),
        "Cloud");
  r.status = detail::cloudInts(status, {s.n, s.K});
  return r;
}

// index [N,M] kInt64 (-1 once the finite points run out), radiusSq [N,M] (the pick's squared distance to the picks before it; infinity
// for the first), minSqdist [N,K] (every point's squared distance to the sample)
struct CloudSample
{
  Tensor index, radiusSq, minSqdist;
};
// M of the K points of every frame by farthest-point sampling from start [N] (undefined: index 0).
inline CloudSample cloudFarthestPoints(const Tensor & points, int64_t M, const Tensor & start = Tensor(), int device = 0)
{
  const char * what = "Cannot sample the cloud!";
  const detail::CloudShape s = detail::cloudShape(points, what);
  if(M < 1 || M > s.K) throw Exception("Cloud", what);
  if(start.defined() && ((start.dtype != kInt64 && start.dtype != kInt32) || start.numel() != s.n)) throw Exception("Cloud", what);
  std::vector<int32_t> index((size_t)(s.n * M));
  CloudSample r{Tensor(), Tensor({s.n, M}), Tensor({s.n, s.K})};
  check(smplpp_cloud_farthest_points(device, s.n, s.K, points.ptr(), M, start.defined() ? start.data_ptr<int32_t>() : nullptr, index.data(),
                                     r.radiusSq.ptr(), r.minSqdist.ptr(), SMPLPP_HOST, nullptr),
        "Cloud");
  r.index = detail::cloudInts(index, {s.n, M});
  return r;
}
} // namespace smplpp
#endif
