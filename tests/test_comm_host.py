"""The communicator's handle (och_comm in csrc/och_comm.cpp) has one owner at a
time: och::comm_take exchanges it with null, so of a watchdog thread aborting
and an issuing thread failing, aborting or destroying at once, exactly one
hands the RCCL communicator back.  Pinned without a device and without RCCL by
a small C++ program linked against liboch_gpu.so, over a fake handle that is
never dereferenced.

The same driver, compiled with -DOCH_COMM_HOST_STANDALONE together with
och_comm.cpp (no library; the two och_pool.cpp symbols it needs are stubbed
below), is the program to run under -fsanitize=thread.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
ROUNDS, THREADS = 2000, 8

DRIVER = r'''
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "och_gpu.h"

typedef struct ncclComm *ncclComm_t;
namespace och {
och_comm *comm_adopt(ncclComm_t comm, int n_ranks, int rank, int device);
ncclComm_t comm_take(och_comm *comm);
#ifdef OCH_COMM_HOST_STANDALONE             // what och_comm.cpp takes from och_pool.cpp
static thread_local std::string t_error;
int fail(int status, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t_error = buf;
    return status;
}
int report(int status, const char *msg) { return fail(status, "%s", msg); }
#endif
}
#ifdef OCH_COMM_HOST_STANDALONE
extern "C" const char *och_last_error(void) { return och::t_error.c_str(); }
#endif

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 2000, n_threads = argc > 2 ? atoi(argv[2]) : 8;
    const ncclComm_t fake = reinterpret_cast<ncclComm_t>(uintptr_t(0x1000));
    long bad_rounds = 0, info_ok = 0, bad_text = 0, bad_destroy = 0;
    for (int round = 0; round < rounds; ++round) {
        och_comm *c = och::comm_adopt(fake, 1, 0, 0);
        int n = 0, rank = -1, device = -1;
        if (och_comm_info(c, &n, &rank, &device) != OCH_OK || n != 1 || rank != 0 || device != 0) return 3;
        std::atomic<bool> go{false};
        std::atomic<int> ready{0}, got{0}, wrong{0};
        std::vector<std::thread> threads;
        for (int t = 0; t < n_threads; ++t)
            threads.emplace_back([&] {
                ready.fetch_add(1);
                while (!go.load(std::memory_order_acquire)) {}
                const ncclComm_t h = och::comm_take(c);
                if (h == fake) got.fetch_add(1);
                else if (h) wrong.fetch_add(1);
            });
        while (ready.load() < n_threads) std::this_thread::yield();
        go.store(true, std::memory_order_release);
        for (std::thread &t : threads) t.join();
        bad_rounds += got.load() != 1 || wrong.load() != 0;
        if (och_comm_info(c, &n, &rank, &device) == OCH_OK) ++info_ok;
        else if (!strstr(och_last_error(), "NULL or destroyed")) ++bad_text;
        bad_destroy += och_comm_destroy(c) != OCH_OK;
    }
    printf("rounds %d threads %d bad_rounds %ld info_ok %ld bad_text %ld bad_destroy %ld\n", rounds, n_threads,
           bad_rounds, info_ok, bad_text, bad_destroy);
    return 0;
}
'''


@pytest.fixture(scope="module")
def driver(ort, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    libdir = Path(ort.load()._name).resolve().parent
    tmp = tmp_path_factory.mktemp("comm_host")
    src, exe = tmp / "comm_host.cpp", tmp / "comm_host"
    src.write_text(DRIVER)
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{ROOT / 'include'}", str(src), f"-L{libdir}", "-loch_gpu",
                         f"-Wl,-rpath,{libdir}", "-pthread", "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return exe


def test_one_thread_takes_the_handle(driver):
    run = subprocess.run([str(driver), str(ROUNDS), str(THREADS)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    words = run.stdout.split()
    got = dict(zip(words[0::2], map(int, words[1::2])))
    assert got["rounds"] == ROUNDS and got["threads"] == THREADS
    assert got["bad_rounds"] == 0            # exactly one thread per round received the handle, none a wrong one
    assert got["info_ok"] == 0               # the communicator then reports itself destroyed,
    assert got["bad_text"] == 0              # with the "NULL or destroyed" text,
    assert got["bad_destroy"] == 0           # and och_comm_destroy (nothing left to hand to RCCL) returns OCH_OK
