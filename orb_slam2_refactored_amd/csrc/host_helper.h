// LocalBA's helper thread (orbba.hip), standard C++ plus getpid so that a CPU test
// (tests/native/host_helper_check.cpp) shares it.
#pragma once
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

namespace orbamd_host {

// A helper thread per calling thread (round 6): it runs the host half of the structure build (the
// counts, ~50 us at C4) while the calling thread stages and enqueues the problem upload, instead of
// after it.  Started on first use; a process that forked after that (the thread does not exist in the
// child) runs the job on the calling thread.
class HostHelper {
public:
    void post(std::function<void()> f) {
        if (!start()) {   // no helper in this process: run it here
            f();
            done_.store(true, std::memory_order_release);
            return;
        }
        {
            std::lock_guard<std::mutex> lk(m_);
            job_ = std::move(f);
            has_ = true;
            done_.store(false, std::memory_order_relaxed);
        }
        cv_.notify_one();
    }
    void wait() const {   // the job is short: spin (yielding) rather than sleep
        while (!done_.load(std::memory_order_acquire)) std::this_thread::yield();
    }
    ~HostHelper() {
        if (th_.joinable()) {
            if (pid_ != getpid()) {   // forked child: the thread object has no thread behind it
                th_.detach();
                return;
            }
            {
                std::lock_guard<std::mutex> lk(m_);
                quit_ = true;
            }
            cv_.notify_one();
            th_.join();
        }
    }

private:
    bool start() {
        if (th_.joinable()) return pid_ == getpid();
        pid_ = getpid();
        th_ = std::thread([this] { run(); });
        return true;
    }
    void run() {
        std::unique_lock<std::mutex> lk(m_);
        for (;;) {
            cv_.wait(lk, [&] { return has_ || quit_; });
            if (quit_) return;
            std::function<void()> f = std::move(job_);
            has_ = false;
            lk.unlock();
            f();
            done_.store(true, std::memory_order_release);
            lk.lock();
        }
    }
    std::thread th_;
    pid_t pid_ = 0;
    std::mutex m_;
    std::condition_variable cv_;
    std::function<void()> job_;
    bool has_ = false, quit_ = false;
    std::atomic<bool> done_{true};
};

}  // namespace orbamd_host
