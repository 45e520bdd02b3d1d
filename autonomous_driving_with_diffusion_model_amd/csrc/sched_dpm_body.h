// The body of one DPM-Solver++ step at element `e` of DpmArgs `a`, as TEXT, for the reason sched_step_body.h gives: sched.hip
// includes it in dpm_step_kernel and in dpm_step_rows_kernel.  In scope where it is included: a, e, the template's PIN / GUIDE,
// and ROWS with (row_x0, row_moved).
  const adx_dpm_coef& c = a.c;
  const float m = cfg_model_output(a.mo, e, a.total, c.cfg_combine, c.free_scale);
  const float xs = a.x[e];
  float x0 = x0_from(c.prediction_type, c.alpha_s, c.sigma_s, xs, m);
  if (c.clip) x0 = clamp_nan(x0, -c.clip_range, c.clip_range);
  if (GUIDE)      // a moved x0 is the solver's x0 from here on, the history it writes included
    guide_x0(a.guide, a.mo, a.x, e, a.total, a.horizon, a.dim, c.prediction_type, c.alpha_s, c.sigma_s, c.clip, c.clip_range,
             c.cfg_combine, c.free_scale, x0);
  if (ROWS && row_moved) x0 = row_x0;      // the row-wise kernel iterated the waypoint itself
  const float p = c.r * xs, q = c.k * x0;
  float prev = p - q;
  if (c.second_order && a.px0 != nullptr) {
    const float d0 = x0 - a.px0[e];
    const float d1 = c.inv_r0 * d0;
    const float u = c.half_k * d1;
    prev = prev - u;
  }
  if (PIN) {
    // the solver has no noise of its own: the draw exists for the blend alone, at the element's LOGICAL index as in step_kernel
    const float zn = a.pin.known_noise ? noise_normal_at(a.ns, a.slot, a.base + (uint64_t)e) : 0.f;
    prev = pin_blend(a.pin, e, zn, prev);
  }
  if (c.zero_first && first_pose(e, a.horizon, a.dim)) prev = 0.f;
  a.prev[e] = prev;
  a.x0[e] = x0;          // as computed (not zeroed; guided where it moved): the next step's history
