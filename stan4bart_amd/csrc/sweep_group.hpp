// Sweep group: samplers on one device whose solo sweeps (n <= 4 096, one workgroup each) are launched together, one workgroup per member
// (k_sbatch*, dev_sweep.inc).  This header is the rendezvous; the launch belongs to the device layer: DevHip launches one batched kernel
// per variant on the group's stream (HipSweepGroup, dev_hip.hip); a device layer without batched kernels (the CPU emulation of the
// device layer under tests/) gets HostSweepGroup below, whose launch runs each member's sweep in turn (SamplerCore drives it).
//
// A member that reaches its sweep arrives with a job and blocks until a launch has taken the job (enqueued it, not run it).  The launch
// happens once every member that is currently inside run() has arrived — members outside run() are not waited for, and a member leaves the
// set of the waited-for on its way out of run() whatever ends it (SamplerCore::GroupRun: RAII) and when it leaves the group.  The wait is bounded: after
// timeout seconds the members present are launched without the straggler (counted).  Batching never changes a result: every member's sweep
// is the one its own launch would have run.
#ifndef S4B_SWEEP_GROUP_HPP
#define S4B_SWEEP_GROUP_HPP

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <exception>
#include <mutex>
#include <stdexcept>
#include <type_traits>
#include <vector>

namespace s4b {

struct GroupJob {
  void* member = nullptr;       // the member: its device layer (DevHip*) or, for HostSweepGroup, its SamplerCore
  int variant = 0;              // which batched kernel (device layer's own numbering)
  void (*run)(void*) = nullptr; // HostSweepGroup: the member's sweep
  std::exception_ptr err;       // set by the launch for this member alone
  bool done = false;
};

class SweepGroup {
 public:
  enum { ST_LAUNCHES = 0, ST_BATCHED = 1, ST_UNBATCHED = 2, ST_TIMEOUTS = 3 };
  SweepGroup(int device, int maxMembers) : device_(device), max_(maxMembers) {
    if (maxMembers < 1 || maxMembers > 256) throw std::invalid_argument("sweep group: max_members must be in 1..256");
  }
  virtual ~SweepGroup() {}
  SweepGroup(const SweepGroup&) = delete;
  SweepGroup& operator=(const SweepGroup&) = delete;
  int device() const { return device_; }
  int max_members() const { return max_; }
  void set_timeout(double seconds) {
    if (!(seconds > 0.0)) throw std::invalid_argument("sweep group: the timeout must be positive");
    std::lock_guard<std::mutex> lk(m_); timeout_ = seconds;
  }
  size_t members() { std::lock_guard<std::mutex> lk(m_); return members_.size(); }
  void join(void* m) {
    std::lock_guard<std::mutex> lk(m_);
    if (std::find(members_.begin(), members_.end(), m) != members_.end()) throw std::invalid_argument("sweep group: the sampler is already a member");
    if ((int)members_.size() >= max_) throw std::invalid_argument("sweep group: the group is full (max_members)");
    members_.push_back(m);
  }
  void leave(void* m) {
    std::lock_guard<std::mutex> lk(m_);
    members_.erase(std::remove(members_.begin(), members_.end(), m), members_.end());
    active_.erase(std::remove(active_.begin(), active_.end(), m), active_.end());
    cv_.notify_all();
  }
  // run() of member m begins / ends.  Only members whose sweeps are batchable are waited for (eligible): the others never arrive.
  void enter_run(void* m, bool eligible) {
    std::lock_guard<std::mutex> lk(m_);
    if (eligible && std::find(active_.begin(), active_.end(), m) == active_.end()) active_.push_back(m);
  }
  void exit_run(void* m) {
    std::lock_guard<std::mutex> lk(m_);
    active_.erase(std::remove(active_.begin(), active_.end(), m), active_.end());
    cv_.notify_all();      // (the members waiting for it may now be complete)
  }
  // Blocks until a launch has taken the job; rethrows the launch's error for this member.
  void arrive(GroupJob& job) {
    std::unique_lock<std::mutex> lk(m_);
    job.done = false; job.err = nullptr;
    pending_.push_back(&job);
    const bool waited = std::find(active_.begin(), active_.end(), job.member) != active_.end();
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::duration<double>(timeout_));
    while (!job.done) {
      if (!waited || complete()) { launch_pending(); break; }      // (a member outside run() — profile_sweep — is a launch of its own)
      if (cv_.wait_until(lk, deadline) == std::cv_status::timeout && !job.done) { ++stats_[ST_TIMEOUTS]; launch_pending(); break; }
    }
    if (job.err) std::rethrow_exception(job.err);
  }
  void count_unbatched(int64_t k) { std::lock_guard<std::mutex> lk(m_); stats_[ST_UNBATCHED] += k; }
  void stats(int64_t out[4]) { std::lock_guard<std::mutex> lk(m_); for (int i = 0; i < 4; ++i) out[i] = stats_[i]; }

 protected:
  // Enqueues the sweeps of jobs (all on this group's device), called with the group's lock held by exactly one thread at a time.  An error
  // that concerns one member goes to its job.err; an exception thrown out of it goes to every job of the launch.
  virtual void launch(std::vector<GroupJob*>& jobs) = 0;

 private:
  bool complete() const {      // every waited-for member has a job pending
    for (void* a : active_) {
      bool in = false;
      for (const GroupJob* j : pending_) in = in || j->member == a;
      if (!in) return false;
    }
    return true;
  }
  void launch_pending() {
    std::vector<GroupJob*> jobs;
    jobs.swap(pending_);
    try { launch(jobs); }
    catch (...) { const std::exception_ptr e = std::current_exception(); for (GroupJob* j : jobs) if (!j->err) j->err = e; }
    ++stats_[ST_LAUNCHES];
    for (GroupJob* j : jobs) { if (!j->err) ++stats_[ST_BATCHED]; j->done = true; }
    cv_.notify_all();
  }
  const int device_, max_;
  double timeout_ = 30.0;
  std::mutex m_;
  std::condition_variable cv_;
  std::vector<void*> members_, active_;
  std::vector<GroupJob*> pending_;
  int64_t stats_[4] = {0, 0, 0, 0};
};

// The launch of a device layer without batched kernels: every member's sweep in turn, in the launching thread (the others wait in
// arrive()); an exception of one member's sweep goes to that member alone.  Results are those of the members' own sweeps.
class HostSweepGroup : public SweepGroup {
 public:
  HostSweepGroup(int device, int maxMembers) : SweepGroup(device, maxMembers) {}
 protected:
  void launch(std::vector<GroupJob*>& jobs) override {
    for (GroupJob* j : jobs) {
      try { j->run(j->member); } catch (...) { j->err = std::current_exception(); }
    }
  }
};

// does the device layer batch sweeps itself (DevHip: join_group, group_eligible, group_create, its own arrival in the persistent launch)?
template <class D, class = void> struct has_native_sweep_group : std::false_type {};
template <class D> struct has_native_sweep_group<D, std::void_t<decltype(&D::join_group)>> : std::true_type {};

}  // namespace s4b

#endif
