// simulation_ops.hip - host side of libkpdi.so, the simulations that need no resident patterns: the kinematical master
// pattern (kinematical.hip) and the geometrical simulations (geometrical.hip), their tables formed on the host
// (kinematical_plan.h, geometrical_plan.h), the orientation sampling that feeds a dictionary (sampling.hip,
// sampling_plan.h), and what is done with the orientations that come back: disorientation angles, zone reduction and
// KAM maps (orientations.hip, orientations_plan.h).
#include "context.h"

using namespace kpdi;

namespace {

// How the single-launch simulations end: the launch between two events, its result to the host (synchronises: the host
// tables have been read), the kernel's time into `counter`.  *launched = what `launch` returned: the caller words it.
template <typename Launch>
int launch_to_host(kpdi_ctx *c, Launch launch, void *dst, const void *d_src, size_t bytes, double *counter, hipError_t *launched) {
  EventPair timer(c, c->profiling != 0);
  HIPCHK(timer.begin());
  *launched = launch();
  (void)timer.end();
  if (*launched != hipSuccess) return KPDI_OK;
  const int rc = results_to_host(c, dst, d_src, bytes);
  float ms = 0.f;
  if (rc == KPDI_OK && timer.elapsed(&ms) == hipSuccess) *counter = ms;
  return rc;
}

}  // namespace

extern "C" {

int kpdi_kinematical_master_pattern(kpdi_ctx *c, const double *unit_vectors, const double *theta, const double *intensity,
                                    int64_t m, int half_size, int hemispheres, double *out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!unit_vectors || !theta || !intensity || !out) return fail(KPDI_EINVAL, "unit_vectors, theta, intensity or out is NULL");
  if (m < 1 || m > INT_MAX) return fail(KPDI_EINVAL, "%lld reflectors: at least one is needed", (long long)m);
  if (half_size < 0 || half_size > kpdi::KIN_MAX_HALF_SIZE)
    return fail(KPDI_EINVAL, "half_size %d: between 0 and %d", half_size, kpdi::KIN_MAX_HALF_SIZE);
  if (!kpdi::kin_hemispheres(hemispheres))
    return fail(KPDI_EINVAL, "hemispheres %d: 0 (upper), 1 (lower) or 2 (both)", hemispheres);
  const kpdi::KinPlan plan = kpdi::kinematical_launch_plan(m, half_size, hemispheres);
  if (!plan.ok) return fail(KPDI_EINVAL, "kinematical master pattern of half_size %d from %lld reflectors: no kernel takes this shape",
                            half_size, (long long)m);
  int rc = use_device(c);
  if (rc) return rc;
  // the pixel directions of the upper hemisphere and the reflector table, on the host with NumPy's operations
  const int size = plan.size;
  std::vector<double> axis((size_t)size), dirs((size_t)plan.pixels * 3), table((size_t)m * kpdi::KIN_ENTRY_DOUBLES);
  for (int i = 0; i < size; ++i) axis[(size_t)i] = kpdi::kin_axis(i, size);
  for (int r = 0; r < size; ++r)
    for (int col = 0; col < size; ++col) kpdi::kin_direction(axis[(size_t)col], axis[(size_t)r], &dirs[((size_t)r * size + col) * 3]);
  const double half_pi = 1.5707963267948966;  // np.pi / 2
  for (int64_t i = 0; i < m; ++i) {
    double *e = &table[(size_t)i * kpdi::KIN_ENTRY_DOUBLES];
    e[0] = unit_vectors[3 * i];
    e[1] = unit_vectors[3 * i + 1];
    e[2] = unit_vectors[3 * i + 2];
    e[3] = intensity[i];
    e[6] = half_pi - theta[i];
    kpdi::kin_screen(e[6], &e[4], &e[5]);
    e[7] = 0.0;
  }
  const size_t out_bytes = (size_t)plan.hemispheres * (size_t)plan.pixels * sizeof(double);
  HIPCHK(c->kin_dirs.reserve(dirs.size() * sizeof(double)));
  HIPCHK(c->kin_table.reserve(table.size() * sizeof(double)));
  HIPCHK(c->kin_out.reserve(out_bytes));
  HIPCHK(hipMemcpyAsync(c->kin_dirs.p, dirs.data(), dirs.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->kin_table.p, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  kpdi::KinLaunch l{};
  l.dirs = c->kin_dirs.as<double>();
  l.table = c->kin_table.as<double>();
  l.m = m;
  l.half_size = half_size;
  l.hemispheres = hemispheres;
  l.out = c->kin_out.as<double>();
  hipError_t e = hipSuccess;
  rc = launch_to_host(c, [&] { return kpdi::launch_kinematical_master_pattern(l, c->stream); }, out, c->kin_out.p, out_bytes,
                      &c->cnt.kinematical_ms, &e);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "kinematical master pattern kernel: %s (half_size %d, %lld reflectors)", hipGetErrorString(e), half_size,
                (long long)m);
  return rc;
}

// the per-point entries of a geometrical simulation, formed on the host (geometrical_plan.h) and uploaded to c->geo_points
static int geometrical_points(kpdi_ctx *c, const double *rotations, int64_t n_points, const double *u_s, const double *a_star,
                              const double *a_direct, const double *pcs, int64_t n_pc) {
  std::vector<double> entries((size_t)n_points * kpdi::GEO_ENTRY_DOUBLES);
  for (int64_t p = 0; p < n_points; ++p)
    kpdi::geo_point_entry(rotations + 4 * p, u_s, a_star, a_direct, pcs + (n_pc == 1 ? 0 : p) * kpdi::GEO_PC_DOUBLES,
                          &entries[(size_t)p * kpdi::GEO_ENTRY_DOUBLES]);
  HIPCHK(c->geo_points.reserve(entries.size() * sizeof(double)));
  HIPCHK(hipMemcpyAsync(c->geo_points.p, entries.data(), entries.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));  // `entries` leaves scope
  return KPDI_OK;
}

static int geometrical_shape_refused(int64_t n_points, int64_t n_pc) {
  if (n_points < 1 || n_points > INT_MAX) return fail(KPDI_EINVAL, "%lld map points: at least one is needed", (long long)n_points);
  if (n_pc != 1 && n_pc != n_points)
    return fail(KPDI_EINVAL, "%lld projection centres for %lld map points: one, or one per point", (long long)n_pc, (long long)n_points);
  return KPDI_OK;
}

int kpdi_geometrical_visibility(kpdi_ctx *c, const double *vectors, int64_t m, int kind, const double *rotations,
                                int64_t n_points, const double *u_s, const double *basis, const double *pcs, int64_t n_pc,
                                uint8_t *flags) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!vectors || !rotations || !u_s || !basis || !pcs || !flags)
    return fail(KPDI_EINVAL, "vectors, rotations, u_s, basis, pcs or flags is NULL");
  if (m < 1 || m > INT_MAX) return fail(KPDI_EINVAL, "%lld features: at least one is needed", (long long)m);
  int rc = geometrical_shape_refused(n_points, n_pc);
  if (rc) return rc;
  if (kind != KPDI_GEOMETRICAL_LINES && kind != KPDI_GEOMETRICAL_ZONE_AXES)
    return fail(KPDI_EINVAL, "kind %d: 0 (lines) or 1 (zone axes)", kind);
  const kpdi::GeoVisPlan plan = kpdi::geometrical_visibility_plan(m, n_points);
  if (!plan.ok) return fail(KPDI_EINVAL, "visibility of %lld features at %lld map points: no kernel takes this shape", (long long)m,
                            (long long)n_points);
  rc = use_device(c);
  if (rc) return rc;
  rc = geometrical_points(c, rotations, n_points, u_s, kind == KPDI_GEOMETRICAL_LINES ? basis : nullptr,
                          kind == KPDI_GEOMETRICAL_ZONE_AXES ? basis : nullptr, pcs, n_pc);
  if (rc) return rc;
  const size_t vec_bytes = (size_t)m * 3 * sizeof(double), partial_bytes = (size_t)plan.grid_y * (size_t)m;
  HIPCHK(c->geo_vec.reserve(vec_bytes));
  HIPCHK(c->geo_flags.reserve(partial_bytes + (size_t)m));
  HIPCHK(hipMemcpyAsync(c->geo_vec.p, vectors, vec_bytes, hipMemcpyHostToDevice, c->stream));
  kpdi::GeoVisLaunch l{};
  l.vec = c->geo_vec.as<double>();
  l.points = c->geo_points.as<double>();
  l.m = m;
  l.n_points = n_points;
  l.kind = kind;
  l.partial = c->geo_flags.as<uint8_t>();
  l.flags = c->geo_flags.as<uint8_t>() + partial_bytes;
  hipError_t e = hipSuccess;
  rc = launch_to_host(c, [&] { return kpdi::launch_geometrical_visibility(l, c->stream); }, flags, l.flags, (size_t)m,
                      &c->cnt.geometrical_visibility_ms, &e);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "geometrical visibility kernel: %s (%lld features, %lld map points)", hipGetErrorString(e), (long long)m,
                (long long)n_points);
  return rc;
}

int kpdi_geometrical_coordinates(kpdi_ctx *c, const double *hkl, int64_t m, const double *uvw, int64_t z,
                                 const double *rotations, int64_t n_points, const double *u_s, const double *a_star,
                                 const double *a_direct, const double *pcs, int64_t n_pc, double r_gnomonic,
                                 uint8_t *line_in_pattern, double *line_gnomonic, double *line_pixel,
                                 uint8_t *zone_in_pattern, double *zone_gnomonic, double *zone_pixel) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!hkl || !rotations || !u_s || !a_star || !a_direct || !pcs || !line_in_pattern || !line_gnomonic || !line_pixel)
    return fail(KPDI_EINVAL, "hkl, rotations, u_s, a_star, a_direct, pcs or a line output is NULL");
  if (m < 1 || m > INT_MAX) return fail(KPDI_EINVAL, "%lld lines: at least one is needed", (long long)m);
  if (z < 0 || z > INT_MAX) return fail(KPDI_EINVAL, "%lld zone axes: none or more", (long long)z);
  if (z > 0 && (!uvw || !zone_in_pattern || !zone_gnomonic || !zone_pixel))
    return fail(KPDI_EINVAL, "uvw or a zone axis output is NULL");
  int rc = geometrical_shape_refused(n_points, n_pc);
  if (rc) return rc;
  rc = use_device(c);
  if (rc) return rc;
  size_t free_bytes = 0, total_bytes = 0;
  HIPCHK(hipMemGetInfo(&free_bytes, &total_bytes));
  const kpdi::GeoCoordPlan plan = kpdi::geometrical_coord_plan(m, z, n_points, free_bytes / 4);
  if (!plan.ok) return fail(KPDI_EINVAL, "coordinates of %lld lines and %lld zone axes at %lld map points: no kernel takes this shape",
                            (long long)m, (long long)z, (long long)n_points);
  rc = geometrical_points(c, rotations, n_points, u_s, a_star, a_direct, pcs, n_pc);
  if (rc) return rc;
  // the outputs of one pass, each at a multiple of 256 bytes
  const size_t P = (size_t)plan.points, M = (size_t)m, Z = (size_t)z;
  const size_t sizes[6] = {P * M * 4 * sizeof(double), P * M * 4 * sizeof(double), P * Z * 2 * sizeof(double),
                           P * Z * 2 * sizeof(double), P * M, P * Z};
  const auto pad256 = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  size_t offset[6], total = 0;
  for (int i = 0; i < 6; ++i) {
    offset[i] = total;
    total += pad256(sizes[i]);
  }
  const size_t hkl_bytes = M * 3 * sizeof(double), uvw_bytes = Z * 3 * sizeof(double);
  const size_t uvw_at = pad256(hkl_bytes);  // uvw follows hkl in c->geo_vec
  HIPCHK(c->geo_out.reserve(total));
  HIPCHK(c->geo_vec.reserve(uvw_at + uvw_bytes));
  char *vec = c->geo_vec.as<char>(), *out = c->geo_out.as<char>();
  HIPCHK(hipMemcpyAsync(vec, hkl, hkl_bytes, hipMemcpyHostToDevice, c->stream));
  if (z > 0) HIPCHK(hipMemcpyAsync(vec + uvw_at, uvw, uvw_bytes, hipMemcpyHostToDevice, c->stream));
  kpdi::EventPair timer(c, c->profiling != 0);  // recorded again in every pass
  double kernel_ms = 0.0;
  hipError_t e = hipSuccess;
  for (int64_t pass = 0; pass < plan.n_passes && e == hipSuccess && rc == KPDI_OK; ++pass) {
    const int64_t p0 = pass * plan.points;
    const size_t np = (size_t)(pass == plan.n_passes - 1 ? plan.tail : plan.points);
    kpdi::GeoCoordLaunch l{};
    l.hkl = reinterpret_cast<const double *>(vec);
    l.uvw = z > 0 ? reinterpret_cast<const double *>(vec + uvw_at) : nullptr;
    l.points = c->geo_points.as<double>() + (size_t)p0 * kpdi::GEO_ENTRY_DOUBLES;
    l.m = m;
    l.z = z;
    l.points_in_pass = (int64_t)np;
    l.r_gnomonic = r_gnomonic;
    l.line_gn = reinterpret_cast<double *>(out + offset[0]);
    l.line_px = reinterpret_cast<double *>(out + offset[1]);
    l.zone_gn = z > 0 ? reinterpret_cast<double *>(out + offset[2]) : nullptr;
    l.zone_px = z > 0 ? reinterpret_cast<double *>(out + offset[3]) : nullptr;
    l.line_in = reinterpret_cast<uint8_t *>(out + offset[4]);
    l.zone_in = z > 0 ? reinterpret_cast<uint8_t *>(out + offset[5]) : nullptr;
    (void)timer.begin();
    e = kpdi::launch_geometrical_coordinates(l, c->stream);
    (void)timer.end();
    if (e != hipSuccess) break;
    const size_t at = (size_t)p0;
    rc = kpdi::results_to_host(c, line_gnomonic + at * M * 4, l.line_gn, np * M * 4 * sizeof(double));
    if (rc == KPDI_OK) rc = kpdi::results_to_host(c, line_pixel + at * M * 4, l.line_px, np * M * 4 * sizeof(double));
    if (rc == KPDI_OK) rc = kpdi::results_to_host(c, line_in_pattern + at * M, l.line_in, np * M);
    if (rc == KPDI_OK && z > 0) rc = kpdi::results_to_host(c, zone_gnomonic + at * Z * 2, l.zone_gn, np * Z * 2 * sizeof(double));
    if (rc == KPDI_OK && z > 0) rc = kpdi::results_to_host(c, zone_pixel + at * Z * 2, l.zone_px, np * Z * 2 * sizeof(double));
    if (rc == KPDI_OK && z > 0) rc = kpdi::results_to_host(c, zone_in_pattern + at * Z, l.zone_in, np * Z);
    float ms = 0.f;
    if (rc == KPDI_OK && timer.elapsed(&ms) == hipSuccess) kernel_ms += ms;
  }
  if (timer.on() && e == hipSuccess && rc == KPDI_OK) c->cnt.geometrical_coordinates_ms = kernel_ms;
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);  // the host copies of hkl / uvw may still be in flight
    return fail(KPDI_EHIP, "geometrical coordinates kernel: %s (%lld lines, %lld zone axes, %lld map points)", hipGetErrorString(e),
                (long long)m, (long long)z, (long long)n_points);
  }
  return rc;
}

// ---- cubochoric sampling of a fundamental zone (sampling.hip) ------------------------------------------------------------

// device memory the sampler may still take.  KPDI_SAMPLING_FREE_BYTES (tests: the refusal at a small grid) replaces the query
static int sampling_free_bytes(size_t *free_bytes) {
  if (const char *e = getenv("KPDI_SAMPLING_FREE_BYTES")) {
    *free_bytes = (size_t)strtoull(e, nullptr, 10);
    return KPDI_OK;
  }
  size_t total_bytes = 0;
  HIPCHK(hipMemGetInfo(free_bytes, &total_bytes));
  return KPDI_OK;
}

// what `buf` has to grow by to hold `bytes` (DevBuf::reserve frees before it allocates)
static size_t sampling_growth(const kpdi::DevBuf &buf, size_t bytes) { return bytes > buf.cap ? bytes - buf.cap : 0; }

static int sampling_inputs_refused(kpdi_ctx *c, int steps, const double *faces, int n_faces) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (steps < 1 || steps > kpdi::SMP_MAX_STEPS)
    return fail(KPDI_EINVAL, "semi_edge_steps %d: between 1 and %d", steps, kpdi::SMP_MAX_STEPS);
  if (n_faces < 0 || n_faces > kpdi::SMP_MAX_FACES)
    return fail(KPDI_EINVAL, "%d faces: between 0 and %d", n_faces, kpdi::SMP_MAX_FACES);
  if (n_faces > 0 && !faces) return fail(KPDI_EINVAL, "faces is NULL");
  return KPDI_OK;
}

static kpdi::SmpFaces sampling_faces(const double *faces, int n_faces) {
  kpdi::SmpFaces f{};
  f.n = n_faces;
  if (n_faces > 0) memcpy(f.f, faces, (size_t)n_faces * kpdi::SMP_FACE_DOUBLES * sizeof(double));
  return f;
}

static bool sampling_counted(const kpdi_ctx *c, int steps, const kpdi::SmpFaces &f) {
  const auto &s = c->smp_counted;
  return s.valid && s.steps == steps && s.faces.n == f.n && memcmp(s.faces.f, f.f, sizeof(f.f)) == 0;
}

// the count pass and the scan: c->smp_offsets and c->smp_counted describe (steps, f) afterwards
static int sampling_count(kpdi_ctx *c, int steps, const kpdi::SmpFaces &f, double *kernel_ms) {
  const kpdi::SmpPlan plan = kpdi::smp_plan(steps);
  c->smp_counted.valid = false;
  size_t free_bytes = 0;
  int rc = sampling_free_bytes(&free_bytes);
  if (rc) return rc;
  const size_t need = sampling_growth(c->smp_counts, plan.count_bytes) + sampling_growth(c->smp_offsets, plan.offset_bytes);
  if (need > free_bytes)
    return fail(KPDI_ENOMEM, "sampling with semi_edge_steps %d: the counts of %lld workgroups need %zu bytes more, %zu bytes of "
                "device memory are free", steps, (long long)plan.blocks, need, free_bytes);
  HIPCHK(c->smp_counts.reserve(plan.count_bytes));
  HIPCHK(c->smp_offsets.reserve(plan.offset_bytes));
  kpdi::SmpLaunch l{};
  l.faces = f;
  l.steps = steps;
  l.counts = c->smp_counts.as<uint32_t>();
  l.offsets = c->smp_offsets.as<int64_t>();
  EventPair timer(c, c->profiling != 0);
  HIPCHK(timer.begin());
  const hipError_t e = kpdi::launch_sampling_count(l, c->stream);
  (void)timer.end();
  if (e != hipSuccess) return fail(KPDI_EHIP, "sampling count kernels: %s (semi_edge_steps %d)", hipGetErrorString(e), steps);
  int64_t kept = 0;
  rc = results_to_host(c, &kept, l.offsets + plan.blocks, sizeof(kept));
  if (rc) return rc;
  float ms = 0.f;
  if (timer.elapsed(&ms) == hipSuccess) *kernel_ms += ms;
  c->smp_counted.valid = true;
  c->smp_counted.steps = steps;
  c->smp_counted.faces = f;
  c->smp_counted.kept = kept;
  return KPDI_OK;
}

int kpdi_sample_fundamental_count(kpdi_ctx *c, int semi_edge_steps, const double *faces, int n_faces, int64_t *count) {
  int rc = sampling_inputs_refused(c, semi_edge_steps, faces, n_faces);
  if (rc) return rc;
  if (!count) return fail(KPDI_EINVAL, "count is NULL");
  rc = use_device(c);
  if (rc) return rc;
  double kernel_ms = 0.0;
  rc = sampling_count(c, semi_edge_steps, sampling_faces(faces, n_faces), &kernel_ms);
  if (rc) return rc;
  if (c->profiling) c->cnt.sampling_ms = kernel_ms;
  *count = c->smp_counted.kept;
  return KPDI_OK;
}

int kpdi_sample_fundamental_fill(kpdi_ctx *c, int semi_edge_steps, const double *faces, int n_faces, double *out,
                                 int64_t capacity, int64_t *count) {
  int rc = sampling_inputs_refused(c, semi_edge_steps, faces, n_faces);
  if (rc) return rc;
  if (!count) return fail(KPDI_EINVAL, "count is NULL");
  if (capacity < 0 || (capacity > 0 && !out)) return fail(KPDI_EINVAL, "out is NULL or capacity %lld is negative", (long long)capacity);
  rc = use_device(c);
  if (rc) return rc;
  const kpdi::SmpFaces f = sampling_faces(faces, n_faces);
  double kernel_ms = 0.0;
  if (!sampling_counted(c, semi_edge_steps, f)) {
    rc = sampling_count(c, semi_edge_steps, f, &kernel_ms);
    if (rc) return rc;
  }
  const int64_t kept = c->smp_counted.kept;
  *count = kept;
  if (kept > capacity)
    return fail(KPDI_EINVAL, "sampling with semi_edge_steps %d keeps %lld orientations, out holds %lld", semi_edge_steps,
                (long long)kept, (long long)capacity);
  if (kept == 0) return KPDI_OK;
  const size_t out_bytes = (size_t)kept * 4 * sizeof(double);
  size_t free_bytes = 0;
  rc = sampling_free_bytes(&free_bytes);
  if (rc) return rc;
  if (sampling_growth(c->smp_out, out_bytes) > free_bytes)
    return fail(KPDI_ENOMEM, "sampling with semi_edge_steps %d: %lld orientations need %zu bytes, %zu bytes of device memory are "
                "free", semi_edge_steps, (long long)kept, out_bytes, free_bytes);
  HIPCHK(c->smp_out.reserve(out_bytes));
  kpdi::SmpLaunch l{};
  l.faces = f;
  l.steps = semi_edge_steps;
  l.counts = c->smp_counts.as<uint32_t>();
  l.offsets = c->smp_offsets.as<int64_t>();
  l.out = c->smp_out.as<double>();
  l.kept = kept;
  hipError_t e = hipSuccess;
  double emit_ms = 0.0;
  rc = launch_to_host(c, [&] { return kpdi::launch_sampling_emit(l, c->stream); }, out, c->smp_out.p, out_bytes, &emit_ms, &e);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "sampling emit kernel: %s (semi_edge_steps %d, %lld orientations)", hipGetErrorString(e), semi_edge_steps,
                (long long)kept);
  if (rc == KPDI_OK && c->profiling) c->cnt.sampling_ms = kernel_ms + emit_ms;
  return rc;
}

// ---- disorientation angles, zone reduction, KAM maps (orientations.hip) ------------------------------------------------

static int orientation_ops(const double *ops, int n_ops, const char *what, kpdi::OriOps *o) {
  if (!ops) return fail(KPDI_EINVAL, "%s is NULL", what);
  if (n_ops < 1 || n_ops > kpdi::ORI_MAX_OPS) return fail(KPDI_EINVAL, "%d operations in %s: between 1 and %d", n_ops, what, kpdi::ORI_MAX_OPS);
  *o = kpdi::OriOps{};
  o->n = n_ops;
  memcpy(o->q, ops, (size_t)n_ops * 4 * sizeof(double));
  return KPDI_OK;
}

// free device memory beyond what the context's buffers of this call already hold
static int orientation_fits(size_t need, size_t held, const char *what) {
  size_t free_bytes = 0, total_bytes = 0;
  HIPCHK(hipMemGetInfo(&free_bytes, &total_bytes));
  if (need > held && need - held > free_bytes)
    return fail(KPDI_ENOMEM, "%s needs %zu bytes of device memory, %zu are held and %zu free", what, need, held, free_bytes);
  return KPDI_OK;
}

static int orientation_upload(kpdi_ctx *c, kpdi::DevBuf &buf, const void *src, size_t bytes) {
  HIPCHK(buf.reserve(bytes));
  HIPCHK(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, c->stream));
  return KPDI_OK;
}

int kpdi_orientation_pairs(kpdi_ctx *c, const double *q1, int64_t rows1, const double *q2, int64_t rows2, int ndim,
                           const int64_t *shape, const int64_t *stride1, const int64_t *stride2, const double *ops1,
                           int n_ops1, const double *ops2, int n_ops2, int degrees, double *out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!q1 || !q2 || !out) return fail(KPDI_EINVAL, "q1, q2 or out is NULL");
  if (rows1 < 1 || rows2 < 1) return fail(KPDI_EINVAL, "%lld and %lld rows: at least one each", (long long)rows1, (long long)rows2);
  if (ndim < 0 || ndim > kpdi::ORI_MAX_DIMS) return fail(KPDI_EINVAL, "%d leading axes: between 0 and %d", ndim, kpdi::ORI_MAX_DIMS);
  if (ndim > 0 && (!shape || !stride1 || !stride2)) return fail(KPDI_EINVAL, "shape, stride1 or stride2 is NULL");
  kpdi::OriPairsLaunch l{};
  int rc = orientation_ops(ops1, n_ops1, "ops1", &l.ops1);
  if (rc) return rc;
  rc = orientation_ops(ops2, n_ops2, "ops2", &l.ops2);
  if (rc) return rc;
  l.shape.nd = ndim;
  int64_t count = 1, last1 = 0, last2 = 0;
  for (int d = 0; d < ndim; ++d) {
    if (shape[d] < 1 || stride1[d] < 0 || stride2[d] < 0 || shape[d] > INT64_MAX / 64 / count)
      return fail(KPDI_EINVAL, "axis %d: length %lld, strides %lld and %lld", d, (long long)shape[d], (long long)stride1[d],
                  (long long)stride2[d]);
    l.shape.dim[d] = shape[d];
    l.shape.stride1[d] = stride1[d];
    l.shape.stride2[d] = stride2[d];
    count *= shape[d];
    if ((stride1[d] && (shape[d] - 1) > (rows1 - 1 - last1) / stride1[d]) || (stride2[d] && (shape[d] - 1) > (rows2 - 1 - last2) / stride2[d]))
      return fail(KPDI_EINVAL, "axis %d of length %lld with strides %lld and %lld leaves an input of %lld and %lld rows", d,
                  (long long)shape[d], (long long)stride1[d], (long long)stride2[d], (long long)rows1, (long long)rows2);
    last1 += (shape[d] - 1) * stride1[d];
    last2 += (shape[d] - 1) * stride2[d];
  }
  if (kpdi::ori_blocks(count) > kpdi::ORI_MAX_TILES) return fail(KPDI_EINVAL, "%lld pairs: more than one launch takes", (long long)count);
  rc = use_device(c);
  if (rc) return rc;
  const size_t b1 = (size_t)rows1 * 32, b2 = (size_t)rows2 * 32, bo = (size_t)count * sizeof(double);
  rc = orientation_fits(b1 + b2 + bo, c->ori_a.cap + c->ori_b.cap + c->ori_out.cap, "the disorientation angles of these pairs");
  if (rc) return rc;
  rc = orientation_upload(c, c->ori_a, q1, b1);
  if (rc == KPDI_OK) rc = orientation_upload(c, c->ori_b, q2, b2);
  if (rc) return rc;
  HIPCHK(c->ori_out.reserve(bo));
  l.q1 = c->ori_a.as<double>();
  l.q2 = c->ori_b.as<double>();
  l.count = count;
  l.degrees = degrees != 0;
  l.out = c->ori_out.as<double>();
  hipError_t e = hipSuccess;
  double ms = 0.0;
  rc = launch_to_host(c, [&] { return kpdi::launch_orientation_pairs(l, c->stream); }, out, l.out, bo, &ms, &e);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);  // the uploads read the caller's arrays
    return fail(KPDI_EHIP, "orientation pairs kernel: %s (%lld pairs)", hipGetErrorString(e), (long long)count);
  }
  if (rc == KPDI_OK && c->profiling) c->cnt.orientation_ms = ms;
  return rc;
}

int kpdi_orientation_outer(kpdi_ctx *c, const double *q1, int64_t n, const double *q2, int64_t m, const double *ops1,
                           int n_ops1, const double *ops2, int n_ops2, int degrees, int dtype_out, void *out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!q1 || !q2 || !out) return fail(KPDI_EINVAL, "q1, q2 or out is NULL");
  if (n < 1 || m < 1 || n > INT64_MAX / 64 / m) return fail(KPDI_EINVAL, "%lld x %lld orientations: at least one each", (long long)n, (long long)m);
  if (dtype_out != KPDI_F64 && dtype_out != KPDI_F32) return fail(KPDI_EINVAL, "dtype_out %d: the angles are float64 or float32", dtype_out);
  kpdi::OriOps o1, o2;
  int rc = orientation_ops(ops1, n_ops1, "ops1", &o1);
  if (rc) return rc;
  rc = orientation_ops(ops2, n_ops2, "ops2", &o2);
  if (rc) return rc;
  int64_t forced = 0;
  if (const char *e = getenv("KPDI_ORIENT_PASS_ROWS")) {
    forced = strtoll(e, nullptr, 10);
    if (forced < 1) return fail(KPDI_EINVAL, "KPDI_ORIENT_PASS_ROWS=%s: a positive number of rows", e);
  }
  rc = use_device(c);
  if (rc) return rc;
  const int elem = dtype_out == KPDI_F64 ? 8 : 4;
  const size_t b1 = (size_t)n * 32, b2 = (size_t)m * 32;
  size_t free_bytes = 0, total_bytes = 0;
  HIPCHK(hipMemGetInfo(&free_bytes, &total_bytes));
  const size_t held = c->ori_a.cap + c->ori_b.cap + c->ori_out.cap, inputs = b1 + b2;
  const size_t room = free_bytes + held > inputs ? free_bytes + held - inputs : 0;
  const kpdi::OriOuterPlan plan = kpdi::ori_outer_plan(n, m, elem, room / 2, forced);
  if (!plan.ok || plan.pass_bytes > room)
    return fail(KPDI_ENOMEM, "the %lld x %lld disorientation angles: the inputs and one pass of rows need more than the %zu "
                "bytes of device memory that are free", (long long)n, (long long)m, free_bytes);
  rc = orientation_upload(c, c->ori_a, q1, b1);
  if (rc == KPDI_OK) rc = orientation_upload(c, c->ori_b, q2, b2);
  if (rc) return rc;
  HIPCHK(c->ori_out.reserve(plan.pass_bytes));
  kpdi::EventPair timer(c, c->profiling != 0);  // recorded again in every pass
  double kernel_ms = 0.0;
  hipError_t e = hipSuccess;
  for (int64_t pass = 0; pass < plan.n_passes && rc == KPDI_OK; ++pass) {
    kpdi::OriOuterLaunch l{};
    l.q1 = c->ori_a.as<double>();
    l.q2 = c->ori_b.as<double>();
    l.n = n;
    l.m = m;
    l.row_first = pass * plan.pass_rows;
    l.pass_rows = pass == plan.n_passes - 1 ? plan.tail_rows : plan.pass_rows;
    l.ops1 = o1;
    l.ops2 = o2;
    l.degrees = degrees != 0;
    l.elem_bytes = elem;
    l.out = c->ori_out.p;
    (void)timer.begin();
    e = kpdi::launch_orientation_outer(l, c->stream);
    (void)timer.end();
    if (e != hipSuccess) break;
    const size_t row_bytes = (size_t)m * (size_t)elem;
    rc = kpdi::results_to_host(c, (char *)out + (size_t)l.row_first * row_bytes, c->ori_out.p, (size_t)l.pass_rows * row_bytes);
    float ms = 0.f;
    if (rc == KPDI_OK && timer.elapsed(&ms) == hipSuccess) kernel_ms += ms;
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    return fail(KPDI_EHIP, "orientation outer kernel: %s (%lld x %lld)", hipGetErrorString(e), (long long)n, (long long)m);
  }
  if (rc == KPDI_OK && timer.on()) c->cnt.orientation_ms = kernel_ms;
  return rc;
}

int kpdi_orientation_reduce(kpdi_ctx *c, const double *q, int64_t n, const double *ops, int n_ops, double *out, int32_t *index) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!q || !out || !index) return fail(KPDI_EINVAL, "q, out or index is NULL");
  if (n < 1 || kpdi::ori_blocks(n) > kpdi::ORI_MAX_TILES) return fail(KPDI_EINVAL, "%lld orientations: at least one is needed", (long long)n);
  kpdi::OriReduceLaunch l{};
  int rc = orientation_ops(ops, n_ops, "ops", &l.ops);
  if (rc) return rc;
  rc = use_device(c);
  if (rc) return rc;
  const size_t bq = (size_t)n * 32, bi = (size_t)n * sizeof(int32_t);
  rc = orientation_fits(2 * bq + bi, c->ori_a.cap + c->ori_out.cap + c->ori_tab.cap, "the zone reduction of these orientations");
  if (rc) return rc;
  rc = orientation_upload(c, c->ori_a, q, bq);
  if (rc) return rc;
  HIPCHK(c->ori_out.reserve(bq));
  HIPCHK(c->ori_tab.reserve(bi));
  l.q = c->ori_a.as<double>();
  l.n = n;
  l.out = c->ori_out.as<double>();
  l.index = c->ori_tab.as<int32_t>();
  hipError_t e = hipSuccess;
  double ms = 0.0;
  rc = launch_to_host(c, [&] { return kpdi::launch_orientation_reduce(l, c->stream); }, out, l.out, bq, &ms, &e);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    return fail(KPDI_EHIP, "orientation reduce kernel: %s (%lld orientations)", hipGetErrorString(e), (long long)n);
  }
  if (rc == KPDI_OK) rc = results_to_host(c, index, l.index, bi);
  if (rc == KPDI_OK && c->profiling) c->cnt.orientation_ms = ms;
  return rc;
}

int kpdi_orientation_kam(kpdi_ctx *c, const double *q, int ny, int nx, const double *ops, int n_ops, const int32_t *offsets,
                         int n_offsets, const uint8_t *in_data, double max_angle, int degrees, double *out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!q || !out) return fail(KPDI_EINVAL, "q or out is NULL");
  if (ny < 1 || nx < 1) return fail(KPDI_EINVAL, "a map of %d x %d points: at least one is needed", ny, nx);
  if (n_offsets < 0 || n_offsets > kpdi::ORI_MAX_OFFSETS || (n_offsets > 0 && !offsets))
    return fail(KPDI_EINVAL, "%d window offsets: between 0 and %d, offsets not NULL", n_offsets, kpdi::ORI_MAX_OFFSETS);
  if (max_angle != max_angle) return fail(KPDI_EINVAL, "max_angle is NaN: negative for no limit");
  kpdi::OriKamLaunch l{};
  int rc = orientation_ops(ops, n_ops, "ops", &l.ops);
  if (rc) return rc;
  rc = use_device(c);
  if (rc) return rc;
  const size_t points = (size_t)ny * (size_t)nx, bq = points * 32, bo = points * sizeof(double), bt = (size_t)n_offsets * 2 * sizeof(int32_t);
  rc = orientation_fits(bq + bo + bt + points, c->ori_a.cap + c->ori_out.cap + c->ori_tab.cap + c->ori_mask.cap, "the KAM map");
  if (rc) return rc;
  rc = orientation_upload(c, c->ori_a, q, bq);
  if (rc == KPDI_OK && n_offsets > 0) rc = orientation_upload(c, c->ori_tab, offsets, bt);
  if (rc == KPDI_OK && in_data) rc = orientation_upload(c, c->ori_mask, in_data, points);
  if (rc) return rc;
  HIPCHK(c->ori_out.reserve(bo));
  l.rot = c->ori_a.as<double>();
  l.ny = ny;
  l.nx = nx;
  l.offsets = n_offsets > 0 ? c->ori_tab.as<int32_t>() : nullptr;
  l.n_offsets = n_offsets;
  l.in_data = in_data ? c->ori_mask.as<uint8_t>() : nullptr;
  l.max_angle = max_angle;
  l.degrees = degrees != 0;
  l.out = c->ori_out.as<double>();
  hipError_t e = hipSuccess;
  double ms = 0.0;
  rc = launch_to_host(c, [&] { return kpdi::launch_orientation_kam(l, c->stream); }, out, l.out, bo, &ms, &e);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    return fail(KPDI_EHIP, "orientation KAM kernel: %s (%d x %d points)", hipGetErrorString(e), ny, nx);
  }
  if (rc == KPDI_OK && c->profiling) c->cnt.orientation_ms = ms;
  return rc;
}

}  // extern "C"
