// capi_multi.cpp — cnl_multi: one caller, several devices.  Contiguous balanced shards of the batch, one handle and one persistent
// host thread per device; every call is the single-handle call of each shard, and the devices never exchange data.
#include "handle.h"

namespace {
void multi_worker(cnl_multi* m, size_t i) {
  (void)hipSetDevice(m->device[i]);  // the thread's current device for its whole life
  uint64_t seen = 0;
  for (;;) {
    std::function<int(size_t)> f;
    {
      std::unique_lock<std::mutex> lk(m->mu);
      m->cv_job.wait(lk, [&] { return m->stop || m->generation != seen; });
      if (m->stop) return;
      seen = m->generation;
      f = m->job;
    }
    const int r = f(i);
    {
      std::lock_guard<std::mutex> lk(m->mu);
      m->rc[i] = r;
      if (r) m->msg[i] = g_err;  // thread-local in the worker: carry it over
      if (--m->pending == 0) m->cv_done.notify_all();
    }
  }
}

// runs f(i) for every shard on the shard's worker thread; the first failure (in shard order) becomes the caller's error
template <class F>
int multi_run(cnl_multi* m, F f) {
  const size_t n = m->h.size();
  {
    std::unique_lock<std::mutex> lk(m->mu);
    m->job = f;
    m->rc.assign(n, CNL_OK);
    m->msg.assign(n, std::string());
    m->pending = n;
    m->generation++;
    m->cv_job.notify_all();
    m->cv_done.wait(lk, [&] { return m->pending == 0; });
    m->job = nullptr;
  }
  for (size_t i = 0; i < n; i++)
    if (m->rc[i]) return fail(m->rc[i], "shard " + std::to_string(i) + " (device " + std::to_string(m->device[i]) + "): " + m->msg[i]);
  return CNL_OK;
}
}  // namespace

extern "C" {

// ---- one caller, several devices: contiguous balanced shards of the batch, one handle + one host thread per
//      device, no collective — the devices never exchange data --------------------------------------------------------------
int cnl_multi_create(cnl_multi** mout, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar, int64_t nequ,
                     int64_t ncon, int64_t batch, const int* devices, int ndev) {
  return cnl_multi_create_ex(mout, N, nnz, rows1, cols1, nvar, nequ, ncon, batch, devices, ndev, nullptr);
}

int cnl_multi_create_ex(cnl_multi** mout, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar, int64_t nequ,
                        int64_t ncon, int64_t batch, const int* devices, int ndev, const cnl_options* opt) {
  if (!mout || !devices) return fail(CNL_ERR_ARG, "null argument");
  *mout = nullptr;
  if (ndev < 1 || ndev > 64 || batch < 1) return fail(CNL_ERR_ARG, "need 1 <= ndev <= 64 and batch >= 1");
  cnl::Tuning o;
  int rc = resolve_options(opt, o);
  if (rc) return rc;
  if (o.float32_refine) return fail(CNL_ERR_ARG, "cnl_multi_create_ex: tuning float32_refine is served on single-device handles only (cnl_create_ex)");
  if ((o.float32_staged || o.float32_latency) && (rc = check_f32_options(o, "cnl_multi_create_ex"))) return rc;   // (the key's own rules; its handles are Float64: nothing else of it is read)
  if ((rc = check_subtree_ladder(o, false, "cnl_multi_create_ex"))) return rc;
  int navail = 0;
  if (hipGetDeviceCount(&navail) != hipSuccess || navail == 0) return fail(CNL_ERR_HIP, "no HIP device available (this backend has no CPU fallback)");
  for (int i = 0; i < ndev; i++) if (devices[i] < 0 || devices[i] >= navail) return fail(CNL_ERR_ARG, "device index out of range");
  cnl_multi* m = new cnl_multi();
  m->N = N; m->nnz = nnz; m->batch = batch;
  const int64_t base = batch / ndev, rem = batch % ndev;
  for (int i = 0; i < ndev; i++) {
    const int64_t cnt = base + (i < rem ? 1 : 0);
    if (cnt == 0) continue;  // more devices than problems: the surplus devices stay idle
    m->start.push_back(i * base + std::min<int64_t>(i, rem));
    m->count.push_back(cnt);
    m->device.push_back(devices[i]);
  }
  // The symbolic analysis runs ONCE per shard size ("done once on host and broadcast"): the plan is reference-counted,
  // every shard's handle uploads its own copy of the index data to its device.  Shard sizes differ by at most one problem: one
  // analysis when the batch divides evenly, two otherwise.
  // (round 4: one analysis per DISTINCT shard size — at most two, the sizes differ by at most one problem — so that every shard
  //  runs exactly the plan cnl_create would pick for its own batch: with the first shard's plan for all, a shard on the other
  //  side of a planning boundary (latency / throughput, split eligibility) got its neighbour's plan)
  cnl_plan* shared[2] = {nullptr, nullptr};
  int64_t shared_count[2] = {-1, -1};
  for (size_t i = 0; i < m->count.size() && !rc; i++) {
    cnl_plan* plan = nullptr;
    if (o.multi_share_plan) {
      const int k = shared_count[0] == m->count[i] ? 0 : (shared_count[1] == m->count[i] ? 1 : (shared_count[0] < 0 ? 0 : 1));
      if (shared_count[k] != m->count[i]) {
        if (shared[k]) { cnl_plan_destroy(shared[k]); shared[k] = nullptr; }   // (a third size: cannot happen with balanced shards)
        shared_count[k] = m->count[i];
      }
      if (!shared[k]) rc = plan_create_tuned(&shared[k], N, nnz, rows1, cols1, nvar, nequ, ncon, m->count[i], o);
      if (!rc) { plan = shared[k]; plan->refs.fetch_add(1); }
    } else {
      rc = plan_create_tuned(&plan, N, nnz, rows1, cols1, nvar, nequ, ncon, m->count[i], o);
    }
    cnl_handle* h = nullptr;
    if (!rc) rc = create_from_plan(&h, plan, rows1, cols1, m->count[i], m->device[i]);  // owns one reference, also when it fails
    if (rc) {
      const std::string keep = g_err;
      for (cnl_plan* p : shared) cnl_plan_destroy(p);
      cnl_multi_destroy(m);
      return fail(rc, "shard " + std::to_string(i) + ": " + keep);
    }
    m->h.push_back(h);
  }
  for (cnl_plan* p : shared) cnl_plan_destroy(p);  // the handles keep theirs
  m->rc.assign(m->h.size(), CNL_OK);
  m->msg.assign(m->h.size(), std::string());
  for (size_t i = 0; i < m->h.size(); i++) m->workers.emplace_back(multi_worker, m, i);
  *mout = m;
  return CNL_OK;
}

int cnl_multi_destroy(cnl_multi* m) {
  if (!m) return CNL_OK;
  {
    std::lock_guard<std::mutex> lk(m->mu);
    m->stop = true;
    m->cv_job.notify_all();
  }
  for (auto& t : m->workers) t.join();
  for (cnl_handle* h : m->h) cnl_destroy(h);
  delete m;
  return CNL_OK;
}

int cnl_multi_shards(const cnl_multi* m, int64_t* nshards, int64_t* start, int64_t* count, int32_t* device) {
  if (!m || !nshards) return fail(CNL_ERR_ARG, "null argument");
  *nshards = (int64_t)m->h.size();
  for (size_t i = 0; i < m->h.size(); i++) {
    if (start) start[i] = m->start[i];
    if (count) count[i] = m->count[i];
    if (device) device[i] = m->device[i];
  }
  return CNL_OK;
}

int cnl_multi_factorize(cnl_multi* m, const double* vals, double eig_tol, int32_t* success, int64_t* npos, int64_t* nzero) {
  if (!m || !vals || !success) return fail(CNL_ERR_ARG, "null argument");
  return multi_run(m, [&](size_t i) {
    const int64_t s = m->start[i];
    return cnl_factorize(m->h[i], vals + s * m->nnz, eig_tol, success + s, npos ? npos + s : nullptr, nzero ? nzero + s : nullptr);
  });
}

int cnl_multi_solve(cnl_multi* m, const double* rhs, double* d) {
  if (!m || !rhs || !d) return fail(CNL_ERR_ARG, "null argument");
  return multi_run(m, [&](size_t i) {
    const int64_t s = m->start[i];
    return cnl_solve(m->h[i], rhs + s * m->N, d + s * m->N);
  });
}

int cnl_multi_newton_system(cnl_multi* m, double* vals, const double* rhs, double* d, const double* rho_old, const double params[9],
                            double* rho, double* rho_old_out, int32_t* nfact, int32_t* success) {
  if (!m || !vals || !rhs || !d || !params || !rho || !rho_old_out || !nfact || !success) return fail(CNL_ERR_ARG, "null argument");
  return multi_run(m, [&](size_t i) {
    const int64_t s = m->start[i];
    return cnl_newton_system(m->h[i], vals + s * m->nnz, rhs + s * m->N, d + s * m->N, rho_old ? rho_old + s : nullptr, params, rho + s,
                             rho_old_out + s, nfact + s, success + s);
  });
}

// ---- device-pointer twins: shard i's arrays live on shard i's device (problem-major, count[i] problems).  The calls only
//      ENQUEUE (from the calling thread, one shard after the other) and return; cnl_multi_synchronize waits for all shards.
//      streams[i] == NULL (or streams == NULL): the shard handle's own stream.
static hipStream_t shard_stream(cnl_multi* m, size_t i, void* const* streams) {
  return streams && streams[i] ? (hipStream_t)streams[i] : m->h[i]->stream;
}

int cnl_multi_factorize_dev(cnl_multi* m, const double* const* d_vals, double eig_tol, int32_t* const* d_success, void* const* streams) {
  if (!m || !d_vals || !d_success) return fail(CNL_ERR_ARG, "null argument");
  for (size_t i = 0; i < m->h.size(); i++) {
    const int rc = cnl_factorize_dev(m->h[i], d_vals[i], eig_tol, d_success[i], shard_stream(m, i, streams));
    if (rc) return fail(rc, "shard " + std::to_string(i) + ": " + g_err);
  }
  return CNL_OK;
}

int cnl_multi_solve_dev(cnl_multi* m, const double* const* d_rhs, double* const* d_d, void* const* streams) {
  if (!m || !d_rhs || !d_d) return fail(CNL_ERR_ARG, "null argument");
  for (size_t i = 0; i < m->h.size(); i++) {
    const int rc = cnl_solve_dev(m->h[i], d_rhs[i], d_d[i], shard_stream(m, i, streams));
    if (rc) return fail(rc, "shard " + std::to_string(i) + ": " + g_err);
  }
  return CNL_OK;
}

int cnl_multi_newton_system_dev(cnl_multi* m, double* const* d_vals, const double* const* d_rhs, double* const* d_d,
                                double* const* d_rho_old, double* const* d_rho, int32_t* const* d_nfact, int32_t* const* d_success,
                                const double params[9], void* const* streams) {
  if (!m || !d_vals || !d_rhs || !d_d || !d_rho_old || !d_rho || !d_nfact || !d_success || !params) return fail(CNL_ERR_ARG, "null argument");
  for (size_t i = 0; i < m->h.size(); i++) {
    const int rc = cnl_newton_system_dev(m->h[i], d_vals[i], d_rhs[i], d_d[i], d_rho_old[i], d_rho[i], d_nfact[i], d_success[i], params,
                                         shard_stream(m, i, streams));
    if (rc) return fail(rc, "shard " + std::to_string(i) + ": " + g_err);
  }
  return CNL_OK;
}

int cnl_multi_synchronize(cnl_multi* m, void* const* streams) {
  if (!m) return fail(CNL_ERR_ARG, "null argument");
  for (size_t i = 0; i < m->h.size(); i++) {
    HIPCHK(hipSetDevice(m->device[i]));
    HIPCHK(hipStreamSynchronize(shard_stream(m, i, streams)));
  }
  return CNL_OK;
}

}  // extern "C"
