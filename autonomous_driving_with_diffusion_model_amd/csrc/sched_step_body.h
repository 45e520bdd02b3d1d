// The body of one DDIM / DDPM step at element `e` of StepArgs `a`, as TEXT: sched.hip includes it in step_kernel (one thread per
// element) and in step_rows_kernel (one wave per row), so the arithmetic is written once and step_kernel's instantiations compile
// from the very tokens they always had -- a call into a shared function, even a forced-inline one, reorders their branches.
// In scope where it is included: a, e, the template's DDPM / RNG / PIN / GUIDE, and ROWS with (row_x0, row_moved): the x0 a
// row-wise kernel iterated for this element and whether it moved (constants false in step_kernel: no code).
  const adx_step_coef& c = a.c;
  const float m = cfg_model_output(a.mo, e, a.total, c.cfg_combine, c.free_scale);
  const float xs = a.x[e];
  const float sa = c.sqrt_alpha_t, sb = c.sqrt_beta_t;
  float x0 = x0_from(c.prediction_type, sa, sb, xs, m);
  float eps;
  if (c.prediction_type == ADX_PRED_EPSILON) {
    eps = m;
  } else if (c.prediction_type == ADX_PRED_SAMPLE) {
    const float p = sa * x0;
    eps = (xs - p) / sb;
  } else {
    const float p2 = sa * m, q2 = sb * xs;
    eps = p2 + q2;
  }
  if (c.clip) x0 = clamp_nan(x0, -c.clip_range, c.clip_range);
  bool moved = false;
  if (GUIDE)
    moved = guide_x0(a.guide, a.mo, a.x, e, a.total, a.horizon, a.dim, c.prediction_type, sa, sb, c.clip, c.clip_range, c.cfg_combine,
                     c.free_scale, x0);
  if (ROWS && row_moved) {      // the row-wise kernel iterated the waypoint itself
    x0 = row_x0;
    moved = true;
  }
  const bool known = c.inpaint && a.tgt != nullptr && a.mask != nullptr;
  float zn;
  if (RNG) {
    // the element's index in the LOGICAL tensor, not in this launch: a shard of rows draws what the full batch draws there
    const bool need = c.add_noise || (known && c.known_noise) || (PIN && a.pin.known_noise);
    zn = need ? noise_normal_at(a.ns, a.slot, a.base + (uint64_t)e) : 0.f;
  } else {
    zn = (a.z != nullptr) ? a.z[e] : 0.f;
  }
  float prev;
  if (!DDPM) {
    if (c.use_clipped_model_output || ((GUIDE || ROWS) && moved)) {      // a moved x0 re-derives its eps
      const float p = sa * x0;
      eps = (xs - p) / sb;
    }
    const float dir = c.c_dir * eps;
    const float p = c.c_x0 * x0;
    prev = p + dir;
    if (c.inpaint) {
      prev = prev + c.c_const;
      if (known) prev = repaint_blend(a.tgt, a.mask, e, c.c_known, c.c_known_noise, c.known_noise, zn, prev);
    }
    if (c.add_noise) {
      const float nz = c.c_noise * zn;
      prev = prev + nz;
    }
  } else {
    const float p = c.c_x0 * x0, q = c.c_x * xs;
    prev = p + q;
    if (c.add_noise) {
      const float nz = c.c_noise * zn;
      prev = prev + nz;
    }
    if (known) prev = repaint_blend(a.tgt, a.mask, e, c.c_known, c.c_known_noise, c.known_noise, zn, prev);
  }
  if (PIN) prev = pin_blend(a.pin, e, zn, prev);      // the step's own z: no second draw
  if (c.zero_first && first_pose(e, a.horizon, a.dim)) prev = 0.f;
  a.prev[e] = prev;
  if (a.x0 != nullptr) a.x0[e] = x0;          // as computed (guided where it moved): never pinned
