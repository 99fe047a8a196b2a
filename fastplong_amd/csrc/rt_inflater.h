/* rt_inflater.h -- inflate without a context: a handle of its own for BGZF blocks (bgzf_inflate.h) and for one long deflate stream
   (gzip_inflate.h). */
#pragma once

/* ---- BGZF inflate (bgzf_inflate.h): a handle of its own, no context ---- */
struct fpl_inflater {
    int device = -1;
    Stream stream;
    DevBuf<u8> d_comp, d_out;
    DevBuf<fpl_bgzf_block> d_blocks;
    DevBuf<u32> d_next; /* the kernel's work counter */
    int n_cu = 0;
    std::vector<std::pair<uint64_t, uint64_t>> runs; /* output ranges to bring back, merged */
    /* fpl_inflate_gzip (gzip_inflate.h): the chunks' records, their rooms of 16-bit elements, the 32 KiB windows, the result */
    DevBuf<GzipChunk> d_chunks;
    DevBuf<unsigned short> d_room;
    DevBuf<u8> d_wins;
    DevBuf<fpl_gzip_window> d_res;
};

fpl_inflater* fpl_inflater_create(int32_t device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    fpl_inflater* inf = new (std::nothrow) fpl_inflater();
    if (!inf) return nullptr;
    inf->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || inf->stream.create() != hipSuccess ||
        inf->d_next.alloc(1) != hipSuccess) {
        fpl_inflater_destroy(inf);
        return nullptr;
    }
    inf->n_cu = prop.multiProcessorCount;
    return inf;
}

void fpl_inflater_destroy(fpl_inflater* inf) {
    if (!inf) return;
    if (inf->device >= 0) (void)hipSetDevice(inf->device);
    if (inf->stream) (void)hipStreamSynchronize(inf->stream);
    delete inf; /* (the stream and the buffers go with it) */
}

int fpl_inflate_bgzf(fpl_inflater* inf, const uint8_t* comp, uint64_t comp_bytes, fpl_bgzf_block* blocks, uint32_t n_blocks, uint8_t* out,
                     uint64_t out_bytes) {
    if (!inf) return FPL_ERR_ARG;
    if (n_blocks == 0) return FPL_OK;
    if (!blocks || (comp_bytes && !comp) || (out_bytes && !out)) return FPL_ERR_ARG;
    if (!bgzf_blocks_ok(blocks, n_blocks, comp_bytes, &out_bytes, nullptr)) return FPL_ERR_ARG;
    inf->runs.clear();
    for (uint32_t i = 0; i < n_blocks; i++)
        if (blocks[i].isize) inf->runs.emplace_back(blocks[i].out_off, blocks[i].out_off + blocks[i].isize);
    std::sort(inf->runs.begin(), inf->runs.end());
    size_t n_runs = 0;
    for (const auto& r : inf->runs) { /* ranges that touch are one copy: a reader's window comes back in one */
        if (n_runs && r.first <= inf->runs[n_runs - 1].second)
            inf->runs[n_runs - 1].second = std::max(inf->runs[n_runs - 1].second, r.second);
        else
            inf->runs[n_runs++] = r;
    }
    FPL_HIP_RC(hipSetDevice(inf->device));
    FPL_HIP_RC(inf->d_comp.grow((size_t)comp_bytes + 1, 4096));
    FPL_HIP_RC(inf->d_out.grow((size_t)out_bytes + 1, 4096));
    FPL_HIP_RC(inf->d_blocks.grow(n_blocks, 64));
    hipStream_t s = inf->stream;
    if (comp_bytes) FPL_HIP_RC(hipMemcpyAsync(inf->d_comp.ptr, comp, comp_bytes, hipMemcpyHostToDevice, s));
    FPL_HIP_RC(hipMemcpyAsync(inf->d_blocks.ptr, blocks, sizeof(fpl_bgzf_block) * (size_t)n_blocks, hipMemcpyHostToDevice, s));
    FPL_HIP_RC(bgzf_inflate_enqueue(inf->d_comp.ptr, inf->d_blocks.ptr, n_blocks, inf->d_out.ptr, inf->d_next.ptr, (u32)inf->n_cu, s));
    FPL_HIP_RC(hipGetLastError());
    for (size_t k = 0; k < n_runs; k++)
        FPL_HIP_RC(hipMemcpyAsync(out + inf->runs[k].first, inf->d_out.ptr + inf->runs[k].first, inf->runs[k].second - inf->runs[k].first,
                                  hipMemcpyDeviceToHost, s));
    FPL_HIP_RC(hipMemcpyAsync(blocks, inf->d_blocks.ptr, sizeof(fpl_bgzf_block) * (size_t)n_blocks, hipMemcpyDeviceToHost, s));
    FPL_HIP_RC(hipStreamSynchronize(s));
    return FPL_OK;
}

int fpl_inflate_gzip(fpl_inflater* inf, const uint8_t* comp, uint64_t comp_bytes, uint64_t start_bit, const uint8_t* dict, uint32_t dict_len,
                     uint8_t* out, uint64_t out_cap, uint32_t chunk_bytes, fpl_gzip_window* res) {
    GzipJob job;
    if (!inf || !res || !comp || (dict_len && !dict) || (out_cap && !out) ||
        !gzip_plan(job, comp_bytes, start_bit, dict_len, out_cap, chunk_bytes)) /* every argument, before anything is enqueued */
        return FPL_ERR_ARG;
    const uint64_t skip = start_bit >> 3;
    const size_t room = (size_t)job.n_chunks * job.room_per_chunk + job.room0_extra;
    const size_t out_room = (size_t)std::min<uint64_t>(out_cap, room); /* (a byte per element at most) */
    FPL_HIP_RC(hipSetDevice(inf->device));
    FPL_HIP_RC(inf->d_comp.grow((size_t)job.comp_len + 1, 4096));
    FPL_HIP_RC(inf->d_out.grow(out_room + 1, 4096));
    FPL_HIP_RC(inf->d_chunks.grow(job.n_chunks, 64));
    FPL_HIP_RC(inf->d_room.grow(room, 4096));
    FPL_HIP_RC(inf->d_wins.grow(((size_t)job.n_chunks + 1) * GZIP_WINDOW, 4096));
    if (!inf->d_res.ptr) FPL_HIP_RC(inf->d_res.alloc(1));
    job.comp = inf->d_comp.ptr;
    job.chunks = inf->d_chunks.ptr;
    job.room = inf->d_room.ptr;
    job.wins = inf->d_wins.ptr;
    job.out = inf->d_out.ptr;
    job.res = inf->d_res.ptr;
    job.out_cap = out_room;
    hipStream_t s = inf->stream;
    FPL_HIP_RC(hipMemcpyAsync(inf->d_comp.ptr, comp + skip, job.comp_len, hipMemcpyHostToDevice, s));
    FPL_HIP_RC(hipMemsetAsync(inf->d_wins.ptr, 0, GZIP_WINDOW, s));
    if (dict_len) FPL_HIP_RC(hipMemcpyAsync(inf->d_wins.ptr + (GZIP_WINDOW - dict_len), dict, dict_len, hipMemcpyHostToDevice, s));
    gzip_enqueue(job, (u32)inf->n_cu, s);
    FPL_HIP_RC(hipGetLastError());
    /* the result first: it says how many bytes to bring back */
    FPL_HIP_RC(hipMemcpyAsync(res, inf->d_res.ptr, sizeof(fpl_gzip_window), hipMemcpyDeviceToHost, s));
    FPL_HIP_RC(hipStreamSynchronize(s));
    if (res->status == FPL_GZIP_OK && res->out_bytes) {
        if (res->out_bytes > out_room) return FPL_ERR_HIP; /* (cannot be: k_gzip_windows checks every chunk against out_cap) */
        FPL_HIP_RC(hipMemcpyAsync(out, inf->d_out.ptr, res->out_bytes, hipMemcpyDeviceToHost, s));
        FPL_HIP_RC(hipStreamSynchronize(s));
    }
    res->end_bit += 8 * skip;
    return FPL_OK;
}
