// C ABI, multi-GPU frame assembly (crt_ctx.h maps the units): the RCCL gather and the host-memory exchange.
#include "crt_ctx.h"

#include <rccl/rccl.h> // types and prototypes only: the library is dlopen'ed by crt_comm_init (no link-time dependency)

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <thread>

using namespace crtapi;

// ------------------------------------------------------------------------------------------- native RCCL gather
// One process per GPU; every rank renders its macro tiles into a tile-major staging buffer, ONE ncclAllGather per frame moves
// them over xGMI (1 044 480 bytes per rank at 1080p / 8 GPUs, each rank's 7 inbound messages on 7 different links), the
// untile kernel rebuilds the row-major frame: all on the context's stream, no host synchronisation in between.
// RCCL is resolved at run time (dlopen): a process that already carries an RCCL (torch's librccl.so.1) shares that copy, a
// C++-only process takes /opt/rocm/lib's; a process that never calls crt_comm_* needs none.
namespace {
struct RcclApi {
    void* handle = nullptr;
    ncclResult_t (*getUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*commInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*commDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*allGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*getErrorString)(ncclResult_t) = nullptr;
    std::string error;
};

// loaded once, whichever thread asks first (the initialiser of a function-local static runs exactly once; later callers wait for it)
RcclApi loadRccl()
{
    RcclApi api;
    for (const char* name : { "librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so" }) {
        api.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (api.handle) break;
    }
    if (!api.handle) {
        const char* why = dlerror(); // may be NULL
        api.error = std::string("cannot load RCCL (librccl.so.1): ") + (why ? why : "unknown dlopen error");
        return api;
    }
    api.getUniqueId = reinterpret_cast<decltype(api.getUniqueId)>(dlsym(api.handle, "ncclGetUniqueId"));
    api.commInitRank = reinterpret_cast<decltype(api.commInitRank)>(dlsym(api.handle, "ncclCommInitRank"));
    api.commDestroy = reinterpret_cast<decltype(api.commDestroy)>(dlsym(api.handle, "ncclCommDestroy"));
    api.allGather = reinterpret_cast<decltype(api.allGather)>(dlsym(api.handle, "ncclAllGather"));
    api.getErrorString = reinterpret_cast<decltype(api.getErrorString)>(dlsym(api.handle, "ncclGetErrorString"));
    if (!api.getUniqueId || !api.commInitRank || !api.commDestroy || !api.allGather || !api.getErrorString) {
        api.error = "RCCL library lacks an expected entry point";
        api.handle = nullptr;
    }
    return api;
}

RcclApi& rccl()
{
    static RcclApi api = loadRccl();
    return api;
}

} // namespace

int crt_comm_unique_id(void* id_out)
{
    if (!id_out) return fail(nullptr, CRT_EINVAL, "crt_comm_unique_id: NULL argument");
    RcclApi& api = rccl();
    if (!api.handle) return fail(nullptr, CRT_ENODEVICE, "%s", api.error.c_str());
    ncclUniqueId id;
    const ncclResult_t r = api.getUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, CRT_EHIP, "ncclGetUniqueId failed: %s", api.getErrorString(r));
    static_assert(sizeof(id) == CRT_COMM_ID_BYTES, "crt_hip.h states the size of an RCCL unique id");
    std::memcpy(id_out, &id, sizeof(id));
    return CRT_OK;
}

int crt_comm_init(crt_ctx* c, uint32_t rank, uint32_t n_ranks, const void* unique_id)
{
    if (!c) return CRT_EINVAL;
    if (!unique_id || n_ranks == 0 || rank >= n_ranks) return fail(c, CRT_EINVAL, "crt_comm_init: bad arguments (rank %u of %u)", rank, n_ranks);
    if (c->dist.comm) return fail(c, CRT_ESTATE, "crt_comm_init: the context already has a communicator (crt_comm_destroy first)");
    RcclApi& api = rccl();
    if (!api.handle) return fail(c, CRT_ENODEVICE, "%s", api.error.c_str());
    HIP_TRY(c, hipSetDevice(c->device));
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    const ncclResult_t r = api.commInitRank(&c->dist.comm, static_cast<int>(n_ranks), id, static_cast<int>(rank));
    if (r != ncclSuccess) {
        c->dist.comm = nullptr;
        return fail(c, CRT_EHIP, "ncclCommInitRank(rank %u of %u) failed: %s", rank, n_ranks, api.getErrorString(r));
    }
    c->dist.rank = rank;
    c->dist.ranks = n_ranks;
    return CRT_OK;
}

// ---- the same frame assembly with shared host memory as the transport: for ranks that share ONE GPU (RCCL refuses that), i.e. for
// rehearsing the multi-rank path on a one-GPU machine, and as a fallback where RCCL cannot be loaded.  A POSIX shared-memory object
// holds a header (arrival counter + generation of a sense-reversing barrier) and the ranks' tile slices; per frame: copy the own
// slice in, barrier, copy all slices out, barrier.  Never a measurement of anything.
struct HostExchange {
    struct Header {
        std::atomic<uint32_t> magic, arrive, generation;
        uint32_t nRanks;
        uint64_t capacity;
    };
    static constexpr uint32_t kMagic = 0x43525431u;
    static constexpr size_t kDataAt = 4096;
    int fd = -1;
    void* map = nullptr;
    size_t bytes = 0;
    std::string name;
    bool owner = false;
    Header* header() const { return static_cast<Header*>(map); }
    unsigned char* data() const { return static_cast<unsigned char*>(map) + kDataAt; }
    bool barrier(uint32_t n) const // false: a peer did not arrive within a minute
    {
        Header* h = header();
        const uint32_t gen = h->generation.load(std::memory_order_acquire);
        if (h->arrive.fetch_add(1, std::memory_order_acq_rel) + 1 == n) {
            h->arrive.store(0, std::memory_order_relaxed);
            h->generation.fetch_add(1, std::memory_order_acq_rel);
            return true;
        }
        const auto t0 = std::chrono::steady_clock::now();
        while (h->generation.load(std::memory_order_acquire) == gen) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) return false;
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        return true;
    }
    void close()
    {
        if (map) munmap(map, bytes);
        if (fd >= 0) ::close(fd);
        if (owner && !name.empty()) shm_unlink(name.c_str());
        map = nullptr;
        fd = -1;
    }
};

int crt_comm_init_host(crt_ctx* c, uint32_t rank, uint32_t n_ranks, const char* name)
{
    if (!c) return CRT_EINVAL;
    if (!name || name[0] != '/' || n_ranks == 0 || rank >= n_ranks) return fail(c, CRT_EINVAL, "crt_comm_init_host: bad arguments (rank %u of %u, name must start with '/')", rank, n_ranks);
    if (c->dist.comm || c->dist.hostComm) return fail(c, CRT_ESTATE, "crt_comm_init_host: the context already has a communicator (crt_comm_destroy first)");
    std::unique_ptr<HostExchange> x(new HostExchange);
    x->name = name;
    x->bytes = HostExchange::kDataAt + (size_t(1) << 28); // room for a 8K RGBA8 frame; pages are only taken when touched
    if (rank == 0) {
        x->fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
        if (x->fd < 0) return fail(c, CRT_EIO, "crt_comm_init_host: cannot create shared memory '%s': %s", name, std::strerror(errno));
        x->owner = true;
        if (ftruncate(x->fd, static_cast<off_t>(x->bytes)) != 0) {
            const int e = errno;
            x->close();
            return fail(c, CRT_EIO, "crt_comm_init_host: cannot size '%s': %s", name, std::strerror(e));
        }
    } else {
        for (int tries = 0; tries < 6000 && x->fd < 0; tries++) { // up to 60 s for rank 0 to come up
            x->fd = shm_open(name, O_RDWR, 0600);
            if (x->fd < 0) std::this_thread::sleep_for(std::chrono::milliseconds(10));
        }
        if (x->fd < 0) return fail(c, CRT_EIO, "crt_comm_init_host: rank %u found no shared memory '%s'", rank, name);
        struct stat st;
        for (int tries = 0; tries < 6000; tries++) { // ... and to size it
            if (fstat(x->fd, &st) == 0 && static_cast<size_t>(st.st_size) >= x->bytes) break;
            std::this_thread::sleep_for(std::chrono::milliseconds(10));
        }
    }
    x->map = mmap(nullptr, x->bytes, PROT_READ | PROT_WRITE, MAP_SHARED, x->fd, 0);
    if (x->map == MAP_FAILED) {
        const int e = errno;
        x->map = nullptr;
        x->close();
        return fail(c, CRT_EIO, "crt_comm_init_host: cannot map '%s': %s", name, std::strerror(e));
    }
    HostExchange::Header* h = x->header();
    if (rank == 0) {
        h->arrive.store(0);
        h->generation.store(0);
        h->nRanks = n_ranks;
        h->capacity = x->bytes - HostExchange::kDataAt;
        h->magic.store(HostExchange::kMagic, std::memory_order_release);
    } else {
        int tries = 0;
        while (h->magic.load(std::memory_order_acquire) != HostExchange::kMagic && tries++ < 6000) std::this_thread::sleep_for(std::chrono::milliseconds(10));
        if (h->magic.load(std::memory_order_acquire) != HostExchange::kMagic || h->nRanks != n_ranks) {
            x->close();
            return fail(c, CRT_EIO, "crt_comm_init_host: '%s' is not this launch's exchange (%u ranks expected)", name, n_ranks);
        }
    }
    if (!x->barrier(n_ranks)) { // collective, like crt_comm_init: everybody is attached before anybody goes on (and before rank 0 may unlink)
        x->close();
        return fail(c, CRT_EIO, "crt_comm_init_host: not all %u ranks arrived within a minute", n_ranks);
    }
    c->dist.hostComm = x.release();
    c->dist.rank = rank;
    c->dist.ranks = n_ranks;
    return CRT_OK;
}

int crt_comm_destroy(crt_ctx* c)
{
    if (!c) return CRT_EINVAL;
    if (c->dist.hostComm) {
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        c->dist.hostComm->close();
        delete c->dist.hostComm;
        c->dist.hostComm = nullptr;
        c->dist.ranks = 0;
        return CRT_OK;
    }
    if (!c->dist.comm) return CRT_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    const ncclResult_t r = rccl().commDestroy(c->dist.comm);
    c->dist.comm = nullptr;
    c->dist.ranks = 0;
    return r == ncclSuccess ? CRT_OK : fail(c, CRT_EHIP, "ncclCommDestroy failed: %s", rccl().getErrorString(r));
}

int crt_comm_info(const crt_ctx* c, uint32_t* rank, uint32_t* n_ranks)
{
    if (!c) return CRT_EINVAL;
    if (rank) *rank = c->dist.rank;
    if (n_ranks) *n_ranks = c->dist.ranks; // 0: no communicator
    return CRT_OK;
}

int crt_render_frame_distributed(crt_ctx* c, uint32_t w, uint32_t h, void* d_rgba8, uint8_t* host_rgba8, crt_frame_stats* stats)
{
    int rc = refuseWhitted(c, "crt_render_frame_distributed");
    if (rc == CRT_OK) rc = checkRenderable(c, w, h);
    if (rc) return rc;
    if (!c->dist.comm && !c->dist.hostComm) return fail(c, CRT_ESTATE, "crt_render_frame_distributed: no communicator (crt_comm_init first)");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t n = c->dist.ranks, slots = crt_tile_slots(w, h, n);
    const size_t per = static_cast<size_t>(slots) * crt::kTile * crt::kTile * 4; // bytes each rank contributes
    crt_ctx::DistSlot& d = c->dist.slot[c->dist.serial++ % crt_ctx::kRing];
    if ((rc = ensureBuffer(c, &d.stage, &d.stageBytes, per)) != CRT_OK) return rc;
    if ((rc = ensureBuffer(c, &d.gathered, &d.gatheredBytes, per * n)) != CRT_OK) return rc;
    void* frame = d_rgba8;
    if (!frame) {
        if ((rc = ensureBuffer(c, &d.frame, &d.frameBytes, static_cast<size_t>(w) * h * 4)) != CRT_OK) return rc;
        frame = d.frame;
    }
    // the slot's previous frame (4 frames ago) may have been issued on another stream: order behind it on the GPU
    HIP_TRY(c, d.done.wait(c->stream, false));
    crt_frame_stats local;
    rc = crt_render_tiles_device(c, w, h, c->dist.rank, n, d.stage, stats ? &local : nullptr);
    if (rc) return rc;
    if (c->dist.comm) {
        const ncclResult_t r = rccl().allGather(d.stage, d.gathered, per, ncclUint8, c->dist.comm, c->stream);
        if (r != ncclSuccess) return fail(c, CRT_EHIP, "ncclAllGather failed: %s", rccl().getErrorString(r));
    } else { // through shared host memory: own slice in, everybody waits, all slices out, everybody waits again before the next frame's writes
        HostExchange* x = c->dist.hostComm;
        if (per * n > x->header()->capacity) return fail(c, CRT_EINVAL, "crt_render_frame_distributed: frame too large for the host exchange");
        HIP_TRY(c, hipMemcpyAsync(x->data() + per * c->dist.rank, d.stage, per, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (!x->barrier(n)) return fail(c, CRT_EIO, "crt_render_frame_distributed: a rank did not deliver its tiles within a minute");
        HIP_TRY(c, hipMemcpyAsync(d.gathered, x->data(), per * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (!x->barrier(n)) return fail(c, CRT_EIO, "crt_render_frame_distributed: a rank did not collect the tiles within a minute");
    }
    rc = crt_untile_device(c, w, h, n, d.gathered, frame);
    if (rc) return rc;
    if (host_rgba8) HIP_TRY(c, hipMemcpyAsync(host_rgba8, frame, static_cast<size_t>(w) * h * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, d.done.record(c->stream));
    if (stats || host_rgba8) HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (stats) {
        *stats = local; // kernel_ms and the counters describe this rank's tile launch
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return CRT_OK;
}
