// tor_query_record.inc -- the TorHit record of ray `r` (QRay) for its root `t` on the object `object` of cold record `c`, into the 8
// words at `o`: built once, for the winner, with the reference's operations.  Included by hit_kernel (tor_query.hip) and by
// crossings_kernel's write_record (tor_crossings.hip) with o, c, r, t and object in scope.  Textual, as the descent is: called as a
// function it changes three instructions of every hit kernel.
  double cx, cy, cz;
  centre_at(c, r.time, cx, cy, cz);
  const double px = r.ox + r.dx * t, py = r.oy + r.dy * t, pz = r.oz + r.dz * t;  // rays.nim:24-25 origin + t * direction
  const double inv_r = c[6];                                                     // vec3s.nim:93-94: `/ radius` is `* (1.0 / radius)`
  double nx = (px - cx) * inv_r, ny = (py - cy) * inv_r, nz = (pz - cz) * inv_r;
  const bool front = (r.dx * nx + r.dy * ny + r.dz * nz) < 0.0;  // core.nim:47-49
  if (!front) {
    nx = -nx; ny = -ny; nz = -nz;
  }
  o[0] = px; o[1] = py; o[2] = pz;
  o[3] = nx; o[4] = ny; o[5] = nz;
  o[6] = t;
  o[7] = __longlong_as_double((long long)(((unsigned long long)(front ? 1u : 0u) << 32) | (unsigned)object));
