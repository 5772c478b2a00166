// ray_programs.cu -- device programs for the GPU tests of the ray path of owl/device_runtime.h (optixTrace, the slab
// test, the rope walk, the instance loop, optixReportIntersection with its any-hit dispatch, closest-hit / miss dispatch
// by ray type, the launch index).  Written for the tests; tests/ray_spec.py restates every program in numpy, operation
// for operation in fp32, which is why each body that computes a `t` switches floating-point contraction off.
#include <owl/owl.h>
#include <optix_device.h>

using namespace owl;

struct PrimsGeom {  // both geometry types: boxes c +- half, spheres of radius 0.75 * half inside those boxes
  vec3f *centers;
  float *half;
  int tag;          // which geometry of the scene this is (closest-hit writes it)
  int anyhit_mode;  // 0 accept, 1 ignore odd primitive ids, 2 ignore hit kind 0, 3 accept and terminate the ray
};
struct RayRec {
  float org[3], dir[3];
  float tmin, tmax;
  unsigned type, flags;  // ray type 0 / 1, OPTIX_RAY_FLAG_* word
};
struct HitRec {  // per-ray data, and the record the raygen program writes out
  int prim;
  unsigned inst_id;
  int inst_index, kind;
  unsigned attr0;
  float t;
  int geom;
  int status;  // 0 untouched, 1 closest-hit ran, 2 miss program of ray type 0 ran, 3 miss program of ray type 1 ran
  // written by the intersection program of ray type 1 (that type has no closest-hit program)
  int far_prim;
  unsigned far_inst_id;
  int far_geom;
  float far_t;
};
struct RayParams {
  RayRec *rays;
  HitRec *out;
  unsigned *calls;  // [ray * n_inst + instance index]: intersection-program calls (COUNT pass)
  unsigned *idsum;  // same index: sum of (tag << 12) + primitive id over those calls
  int n_inst;
  int count_mode;
};
struct RaysRayGen {
  OptixTraversableHandle world;
  int n;
};
__constant__ RayParams optixLaunchParams;

static __device__ __forceinline__ unsigned ray_index() {
  const uint3 i = optixGetLaunchIndex(), d = optixGetLaunchDimensions();
  return i.x + i.y * d.x;
}
static __device__ __forceinline__ void count_call(int tag, int prim, bool consistent) {
  const size_t slot = (size_t)ray_index() * optixLaunchParams.n_inst + optixGetInstanceIndex();
  optixLaunchParams.calls[slot] += consistent ? 1u : 0x100000u;  // (a call the program's own slab test refuses poisons the count)
  optixLaunchParams.idsum[slot] += ((unsigned)tag << 12) + (unsigned)prim;
}

OPTIX_BOUNDS_PROGRAM(Prims)(const void *geomData, box3f &bounds, const int primID) {
  const PrimsGeom &g = *(const PrimsGeom *)geomData;
  const vec3f c = g.centers[primID];
  const float h = g.half[primID];
  bounds = box3f(c - h, c + h);
}

// The slab test of the traversal restated on the primitive's own box: the object-space ray, its current interval.
// Reports where the ray enters the box.
OPTIX_INTERSECT_PROGRAM(Boxes)() {
#pragma clang fp contract(off)
  const PrimsGeom &g = owl::getProgramData<PrimsGeom>();
  const int prim = optixGetPrimitiveIndex();
  const vec3f c = g.centers[prim];
  const float h = g.half[prim];
  const float3 ro = optixGetObjectRayOrigin(), rd = optixGetObjectRayDirection();
  const float o[3] = {ro.x, ro.y, ro.z}, d[3] = {rd.x, rd.y, rd.z};
  const float lo[3] = {c.x - h, c.y - h, c.z - h}, hi[3] = {c.x + h, c.y + h, c.z + h};
  float t0 = optixGetRayTmin(), t1 = optixGetRayTmax(), entry = -INFINITY;
  bool hit = true;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (d[a] == 0.f) {
      if (!(lo[a] <= o[a] && o[a] <= hi[a])) hit = false;
    } else {
      const float ta = (lo[a] - o[a]) / d[a], tb = (hi[a] - o[a]) / d[a];
      const float tn = fminf(ta, tb), tf = fmaxf(ta, tb);
      entry = fmaxf(entry, tn);
      t0 = fmaxf(t0, tn);
      t1 = fminf(t1, tf);
      if (!(t0 <= t1)) hit = false;
    }
  }
  if (optixLaunchParams.count_mode) {
    count_call(g.tag, prim, hit);
    return;
  }
  if (hit) optixReportIntersection(entry, 0, (unsigned)prim);
}

struct Roots {
  bool real;
  float t_near, t_far;
};
static __device__ __forceinline__ Roots sphere_roots(const PrimsGeom &g, int prim) {
#pragma clang fp contract(off)
  const vec3f c = g.centers[prim];
  const float r = 0.75f * g.half[prim];
  const float3 o = optixGetObjectRayOrigin(), d = optixGetObjectRayDirection();
  const float x = o.x - c.x, y = o.y - c.y, z = o.z - c.z;
  // around the point of the ray nearest to the centre (parameter s): the half-chord keeps its digits however far
  // away the origin is, where b*b - a*c of the textbook form cancels
  const float a = ((d.x * d.x) + (d.y * d.y)) + (d.z * d.z);
  const float s = -(((x * d.x) + (y * d.y)) + (z * d.z)) / a;
  const float lx = x + (s * d.x), ly = y + (s * d.y), lz = z + (s * d.z);
  const float disc = (r * r) - (((lx * lx) + (ly * ly)) + (lz * lz));
  Roots out = {false, 0.f, 0.f};
  if (!(disc >= 0.f)) return out;
  const float h = sqrtf(disc / a);
  out.real = true;
  out.t_near = s - h;
  out.t_far = s + h;
  return out;
}

// near root with hit kind 0; if that is not accepted, the far root with kind 1
OPTIX_INTERSECT_PROGRAM(Spheres)() {
  const PrimsGeom &g = owl::getProgramData<PrimsGeom>();
  const int prim = optixGetPrimitiveIndex();
  if (optixLaunchParams.count_mode) {
    count_call(g.tag, prim, true);
    return;
  }
  const Roots r = sphere_roots(g, prim);
  if (!r.real) return;
  if (!optixReportIntersection(r.t_near, 0, (unsigned)prim)) optixReportIntersection(r.t_far, 1, (unsigned)prim);
}

// ray type 1: the far root only; no closest-hit program serves this type, so the program keeps the record itself
OPTIX_INTERSECT_PROGRAM(SpheresFar)() {
  const PrimsGeom &g = owl::getProgramData<PrimsGeom>();
  const int prim = optixGetPrimitiveIndex();
  const Roots r = sphere_roots(g, prim);
  if (!r.real) return;
  if (optixReportIntersection(r.t_far, 1, (unsigned)prim)) {
    HitRec &h = owl::getPRD<HitRec>();
    h.far_prim = prim;
    h.far_inst_id = optixGetInstanceId();
    h.far_geom = g.tag;
    h.far_t = r.t_far;
  }
}

OPTIX_ANY_HIT_PROGRAM(Prims)() {
  const PrimsGeom &g = owl::getProgramData<PrimsGeom>();
  if (g.anyhit_mode == 1 && (optixGetAttribute_0() & 1u)) optixIgnoreIntersection();
  if (g.anyhit_mode == 2 && optixGetHitKind() == 0) optixIgnoreIntersection();
  if (g.anyhit_mode == 3) optixTerminateRay();
}

OPTIX_CLOSEST_HIT_PROGRAM(Prims)() {
  const PrimsGeom &g = owl::getProgramData<PrimsGeom>();
  HitRec &h = owl::getPRD<HitRec>();
  h.prim = (int)optixGetPrimitiveIndex();
  h.inst_id = optixGetInstanceId();
  h.inst_index = (int)optixGetInstanceIndex();
  h.kind = (int)optixGetHitKind();
  h.attr0 = optixGetAttribute_0();
  h.t = optixGetRayTmax();
  h.geom = g.tag;
  h.status = 1;
}

OPTIX_MISS_PROGRAM(miss0)() {
  HitRec &h = owl::getPRD<HitRec>();
  h.prim = -1;
  h.status = 2;
}
OPTIX_MISS_PROGRAM(miss1)() {
  HitRec &h = owl::getPRD<HitRec>();
  h.prim = -7;
  h.status = 3;
}

static __device__ void shoot(unsigned i) {
  const RaysRayGen &self = owl::getProgramData<RaysRayGen>();
  if (i >= (unsigned)self.n) return;
  const RayRec r = optixLaunchParams.rays[i];
  HitRec h = {-2, 0u, -2, -2, 0u, -2.f, -2, 0, -2, 0u, -2, -2.f};
  const vec3f org(r.org[0], r.org[1], r.org[2]), dir(r.dir[0], r.dir[1], r.dir[2]);
  if (r.type == 1) {
    owl::RayT<1, 2> ray(org, dir, r.tmin, r.tmax);
    owl::traceRay(self.world, ray, h, r.flags);
  } else {
    owl::RayT<0, 2> ray(org, dir, r.tmin, r.tmax);
    owl::traceRay(self.world, ray, h, r.flags);
  }
  optixLaunchParams.out[i] = h;
}

// ray i of a 1-D launch
OPTIX_RAYGEN_PROGRAM(rays1d)() { shoot(optixGetLaunchIndex().x); }
// ray x + y * dims.x of a 2-D launch
OPTIX_RAYGEN_PROGRAM(rays2d)() {
  const vec2i i = owl::getLaunchIndex(), d = owl::getLaunchDims();
  shoot((unsigned)(i.x + i.y * d.x));
}
