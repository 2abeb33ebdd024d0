"""ntcomp_amd -- Python bindings (ctypes) to libntcomp_gpu.so, the MI355X encode/decode
hot path of ntcomp (tmaklin/ntcomp).

The compute runs in the HIP library; this module only marshals buffers.  There is NO CPU
fallback: if the library is missing or no GPU is visible, the GPU entry points raise.

Names mirror the reference's Rust API (src/lib.rs, src/encode.rs) where it has them:
  encode_sequence(nucleotides, ctx)   ~ ntcomp::encode_sequence + encode::encode_dictionary
                                        (lib.rs:163-230, encode.rs:129-166) -> u64 records
  decode_sequence(encoding, ctx)      ~ ntcomp::decode_sequence (lib.rs:254-318)
  Index.build(seqs, k)                ~ kbo::build(.., add_revcomp = true) (main.rs:111-134)
  Index.load(prefix) / .save(prefix)  ~ kbo::index::load_sbwt / serialize_sbwt

Process note: if torch is used in the same process, import torch BEFORE this module so
the library binds to the already-loaded HIP runtime (one runtime per process).
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# NTC_GPU_LIB: an alternative in-tree build (A/B experiments, ntcomp_amd/csrc/Makefile)
LIB_PATH = os.environ.get("NTC_GPU_LIB") or os.path.join(_HERE, "libntcomp_gpu.so")

NTC_OK = 0
STATUS = {
    0: "NTC_OK", 1: "NTC_ERR_INVALID_ARG", 2: "NTC_ERR_INVALID_BASE", 3: "NTC_ERR_EMPTY_READ",
    4: "NTC_ERR_LENGTH", 5: "NTC_ERR_CAPACITY", 6: "NTC_ERR_HIP", 7: "NTC_ERR_NO_INDEX",
    8: "NTC_ERR_FORMAT", 9: "NTC_ERR_IO", 10: "NTC_ERR_UNSUPPORTED", 11: "NTC_ERR_REFERENCE_PANIC",
    12: "NTC_ERR_DIGEST",
}

# every symbol include/ntcomp_gpu.h and include/ntcomp_host.h declare
EXPORTED = [
    "ntc_abi_version", "ntc_ctx_create", "ntc_ctx_destroy", "ntc_last_error", "ntc_ctx_set_stream",
    "ntc_ctx_synchronize", "ntc_ctx_set_option", "ntc_ctx_get_option", "ntc_index_upload", "ntc_index_info", "ntc_encode_batch",
    "ntc_encode_batch_device", "ntc_encode_status", "ntc_decode_batch", "ntc_decode_batch_device",
    "ntc_decode_status", "ntc_last_timing", "ntc_device_alloc", "ntc_device_free", "ntc_memcpy_h2d",
    "ntc_memcpy_d2h", "ntc_debug_matching_statistics", "ntc_build_index", "ntc_index_free",
    "ntc_index_view_of", "ntc_index_save", "ntc_index_save_as", "ntc_index_load", "ntc_synth_genome", "ntc_synth_strains", "ntc_synth_reads", "ntc_minimizer_keys",
    "ntc_file_header", "ntc_write_block", "ntc_read_block", "ntc_buffer_free", "ntc_pack_block",
    "ntc_deflate_block", "ntc_deflate_stream", "ntc_pack_blocks_device", "ntc_deflate_blocks_device",
    "ntc_encode_members", "ntc_inflate_members", "ntc_inflate_members_device", "ntc_encode_pack_batch", "ntc_fastq_parse",
    "ntc_encode_pack_fastq", "ntc_read_block_into", "ntc_read_block_streams", "ntc_unpack_streams",
    "ntc_unpacked_records", "ntc_decode_fasta_unpacked",
    "ntc_fastx_open", "ntc_fastx_next_batch", "ntc_fastx_close", "ntc_fasta_format", "ntc_fastx_next_batch_into",
    "ntc_fastx_set_threads", "ntc_host_threads", "ntc_encode_file", "ntc_decode_fasta",
    "ntc_decode_file", "ntc_build_index_device", "ntc_build_index_device_ex", "ntc_index_set_prefix_precalc",
    "ntc_index_prefix_table", "ntc_index_share", "ntc_index_prepare", "ntc_index_upload_prepared", "ntc_index_prep_free",
    "ntc_encode_exceptions", "ntc_decode_set_exceptions", "ntc_nx_write", "ntc_nx_read", "ntc_encode_file_nx",
    "ntc_decode_file_nx",
    "ntc_encode_qualities", "ntc_decode_set_qualities", "ntc_q_write_header", "ntc_q_write_header2", "ntc_q_deflate_section",
    "ntc_q_write_section", "ntc_q_read", "ntc_encode_file_ex", "ntc_decode_file_ex",
    "ntc_encode_names", "ntc_decode_set_names", "ntc_n_write_header", "ntc_n_deflate_section",
    "ntc_n_write_section", "ntc_n_read", "ntc_encode_file_ex2", "ntc_decode_file_ex2",
    "ntc_encode_digests", "ntc_decode_set_digests", "ntc_decode_digests", "ntc_d_write_header",
    "ntc_d_write_section", "ntc_d_read", "ntc_encode_file_ex3", "ntc_decode_file_ex3",
    "ntc_encode_pack_fastq_paired", "ntc_decode_pair_split", "ntc_encode_file_ex4", "ntc_decode_file_ex4",
    "ntc_decode_set_window", "ntc_decode_file_ex5", "ntc_archive_info", "ntc_encode_file_ex6",
    "ntc_bgzf_bound", "ntc_bgzf_compress", "ntc_bgzf_compress_device", "ntc_bgzf_last", "ntc_decode_file_ex7",
]

# non-ACGT policies (ctx option "non_acgt", include/ntcomp_gpu.h) and the twelve symbols they cover
NON_ACGT = {"error": 0, "mask": 1, "keep": 2}
NX_SYMBOLS = b"N-BDHVRYSWKM"
# ntc_nx_run: an exception run, 24 bytes
NX_RUN = np.dtype([("read", "<u8"), ("pos", "<u4"), ("len", "<u4"), ("sym", "<u4"), ("reserved", "<u4")])


# quality modes (ctx option "qualities", include/ntcomp_codec.h)
QUALITIES = {"drop": 0, "keep": 1, "bin8": 2}
# the quality sections' coder (ctx option "quality_coder"): packed codes, or order-1 rANS on the GPU
QUALITY_CODERS = {"pack": 0, "rans": 1}


def _quality_code(qualities):
    return QUALITIES[qualities] if isinstance(qualities, str) else int(qualities)


def _coder_code(coder):
    return QUALITY_CODERS[coder] if isinstance(coder, str) else int(coder)


# smoothing inside long matches (ctx options "quality_smooth", "quality_smooth_to"): a quality
# inside a long record of at least M bases becomes the target byte; 0 = off
QUALITY_SMOOTH_MIN, QUALITY_SMOOTH_MAX, QUALITY_SMOOTH_DEFAULT = 12, 16777215, 32
QUALITY_SMOOTH_TO = b"I"


def _smooth_code(m):
    """quality_smooth as the option takes it: 0 (off) or M in 12..16777215."""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)):
        raise ValueError(f"quality_smooth must be an integer, not {m!r}")
    if m != 0 and not QUALITY_SMOOTH_MIN <= m <= QUALITY_SMOOTH_MAX:
        raise ValueError(f"quality_smooth must be 0 (off) or {QUALITY_SMOOTH_MIN}..{QUALITY_SMOOTH_MAX}, not {m}")
    return int(m)


def _smooth_to_code(to):
    """quality_smooth_to as the option takes it: one byte in '$'..'~' (bytes, str or int)."""
    if isinstance(to, str):
        to = to.encode("latin-1", errors="replace")
    if isinstance(to, (bytes, bytearray)):
        if len(to) != 1:
            raise ValueError(f"quality_smooth_to must be one byte, not {bytes(to)!r}")
        to = to[0]
    if isinstance(to, bool) or not isinstance(to, (int, np.integer)) or not ord("$") <= to <= ord("~"):
        raise ValueError(f"quality_smooth_to must be a byte in '$'..'~', not {to!r}")
    return int(to)


# name modes (ctx option "names", include/ntcomp_codec.h)
NAMES = {"drop": 0, "keep": 1, "id": 2}
NAME_MAX, NAME_GROUP = 4095, 64


def _names_code(names):
    return NAMES[names] if isinstance(names, str) else int(names)


# paired-end reads (ctx option "paired", include/ntcomp_codec.h): off, pairs with the mate
# check on the ids, pairs without a check
PAIR_MODES = {"off": 0, "ids": 1, "nocheck": 2}


def _pair_code(paired):
    return PAIR_MODES[paired] if isinstance(paired, str) else int(paired)


def _policy_code(non_acgt):
    return NON_ACGT[non_acgt] if isinstance(non_acgt, str) else int(non_acgt)


class NtcError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__(f"{STATUS.get(code, code)}: {msg}")


class IndexView(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_uint64), ("k", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("rows", ctypes.c_void_p * 4), ("C", ctypes.c_uint64 * 4), ("lcs", ctypes.c_void_p)]


class StreamMeta(ctypes.Structure):
    _fields_ = [("num_u64", ctypes.c_uint64), ("encoded_size", ctypes.c_uint64), ("param", ctypes.c_uint64),
                ("offset", ctypes.c_uint64)]


class BlockMeta(ctypes.Structure):
    """ntc_block_meta (include/ntcomp_codec.h): the four packed streams of one block."""
    _fields_ = [("stream", StreamMeta * 4), ("num_records", ctypes.c_uint64), ("n_recs", ctypes.c_uint64),
                ("status", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


class QualMeta(ctypes.Structure):
    """ntc_qual_meta (include/ntcomp_codec.h): the quality section of one block."""
    _fields_ = [("n_reads", ctypes.c_uint64), ("n_quals", ctypes.c_uint64), ("payload_off", ctypes.c_uint64),
                ("payload_bytes", ctypes.c_uint64), ("width", ctypes.c_uint8), ("n_syms", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 6), ("alphabet", ctypes.c_uint8 * 96)]

    @property
    def coder(self):
        """0 pack, 1 rans: the first reserved byte"""
        return int(self.reserved[0])

    @coder.setter
    def coder(self, value):
        self.reserved[0] = int(value)


class NameMeta(ctypes.Structure):
    """ntc_name_meta (include/ntcomp_codec.h): the name section of one block."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_reads", "name_bytes", "mid_bytes", "payload_off", "payload_bytes")]


# digest components (ntc_digest_meta.components, include/ntcomp_codec.h)
DIGEST_SEQ, DIGEST_SYM, DIGEST_QUAL, DIGEST_NAME = 1, 2, 4, 8
DIGEST_COMPONENTS = ("seq", "sym", "qual", "name")


class DigestMeta(ctypes.Structure):
    """ntc_digest_meta (include/ntcomp_codec.h): the content digests of one block."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_reads", "n_bases", "d_seq", "d_sym", "d_qual", "d_name")] + \
               [("components", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


DEFLATE_ENGINES = {"zlib": 0, "libdeflate": 1, "adaptive": 2, "gpu": 3}  # NTC_DEFLATE_* (include/ntcomp_codec.h)


class PipelineOpts(ctypes.Structure):
    _fields_ = [("threads", ctypes.c_int32), ("blocks_per_batch", ctypes.c_int32), ("batch_bases", ctypes.c_uint64),
                ("deflate_engine", ctypes.c_int32), ("host_parse", ctypes.c_int32)]


class PipelineStats(ctypes.Structure):
    _fields_ = [("reads", ctypes.c_uint64), ("bases", ctypes.c_uint64), ("blocks", ctypes.c_uint64),
                ("dropped_blocks", ctypes.c_uint64), ("bytes_out", ctypes.c_uint64), ("parse_s", ctypes.c_double),
                ("gpu_s", ctypes.c_double), ("deflate_s", ctypes.c_double), ("write_s", ctypes.c_double),
                ("wall_s", ctypes.c_double), ("alloc_s", ctypes.c_double), ("first_batch_s", ctypes.c_double),
                ("reader_done_s", ctypes.c_double), ("gpu_done_s", ctypes.c_double), ("threads", ctypes.c_int32), ("gpu_parsed", ctypes.c_int32),
                ("bad_read", ctypes.c_int64), ("error", ctypes.c_char * 256)]


class NxStats(ctypes.Structure):
    """ntc_nx_stats (include/ntcomp_pipeline.h)."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("runs", "bases", "reads", "runs_in_dropped_blocks")]


class FileOpts(ctypes.Structure):
    """ntc_file_opts (include/ntcomp_pipeline.h): both side files of a file-to-file call."""
    _fields_ = [("nx_policy", ctypes.c_int32), ("nx_fd", ctypes.c_int32), ("q_mode", ctypes.c_int32),
                ("q_fd", ctypes.c_int32), ("nx_path", ctypes.c_char_p), ("q_path", ctypes.c_char_p)]


class QStats(ctypes.Structure):
    """ntc_q_stats (include/ntcomp_pipeline.h)."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("sections", "quals", "packed_bytes", "deflated_bytes")]


class FileOpts2(ctypes.Structure):
    """ntc_file_opts2 (include/ntcomp_pipeline.h): all three side files of a file-to-file call."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("nx_policy", ctypes.c_int32), ("nx_fd", ctypes.c_int32),
                ("q_mode", ctypes.c_int32), ("q_fd", ctypes.c_int32), ("nx_path", ctypes.c_char_p),
                ("q_path", ctypes.c_char_p), ("n_mode", ctypes.c_int32), ("n_fd", ctypes.c_int32),
                ("n_path", ctypes.c_char_p)]


class FileOpts3(ctypes.Structure):
    """ntc_file_opts3 (include/ntcomp_pipeline.h): the three side files and the digest file."""
    _fields_ = FileOpts2._fields_ + [("d_mode", ctypes.c_int32), ("d_fd", ctypes.c_int32), ("d_path", ctypes.c_char_p)]


class FileOpts4(ctypes.Structure):
    """ntc_file_opts4 (include/ntcomp_pipeline.h): ntc_file_opts3 and the pairs."""
    _fields_ = FileOpts3._fields_ + [("pair_mode", ctypes.c_int32), ("mate_path", ctypes.c_char_p), ("out_fd2", ctypes.c_int32)]


class FileOpts5(ctypes.Structure):
    """ntc_file_opts5 (include/ntcomp_pipeline.h): ntc_file_opts4 and the range of reads."""
    _fields_ = FileOpts4._fields_ + [("read_first", ctypes.c_uint64), ("read_count", ctypes.c_uint64)]


class FileOpts6(ctypes.Structure):
    """ntc_file_opts6 (include/ntcomp_pipeline.h): ntc_file_opts5 and the engine that inflates a BGZF input."""
    _fields_ = FileOpts5._fields_ + [("inflate_engine", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# who inflates a BGZF input (ntc_file_opts6.inflate_engine)
INFLATE_ENGINES = {"host": 0, "gpu": 1}


class IStats(ctypes.Structure):
    """ntc_i_stats (include/ntcomp_pipeline.h)."""
    _fields_ = [("engine", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("members", ctypes.c_uint64),
                ("bytes", ctypes.c_uint64), ("runs", ctypes.c_uint64), ("fallback_runs", ctypes.c_uint64),
                ("seconds", ctypes.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class FileOpts7(ctypes.Structure):
    """ntc_file_opts7 (include/ntcomp_pipeline.h): ntc_file_opts6 and the format of the decoded output."""
    _fields_ = FileOpts6._fields_ + [("out_format", ctypes.c_int32), ("reserved2", ctypes.c_int32)]


# the format of decode's output (ntc_file_opts7.out_format)
OUT_FORMATS = {"text": 0, "bgzf": 1}


class ZStats(ctypes.Structure):
    """ntc_z_stats (include/ntcomp_pipeline.h)."""
    _fields_ = [("out_format", ctypes.c_uint32), ("reserved", ctypes.c_uint32)] + \
               [(n, ctypes.c_uint64) for n in ("members", "text_bytes", "bytes", "chunks_stored", "chunks_huffman",
                                               "chunks_matches")] + [("seconds", ctypes.c_double)]

    def as_dict(self):
        return {k: (float(self.seconds) if k == "seconds" else int(getattr(self, k))) for k, _ in self._fields_ if k != "reserved"}


class RStats(ctypes.Structure):
    """ntc_r_stats (include/ntcomp_pipeline.h)."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("blocks_total", "reads_total", "first_block", "blocks_read",
                                               "reads_written", "head_skipped", "tail_skipped")]


class ArchiveBlock(ctypes.Structure):
    """ntc_archive_block (include/ntcomp_pipeline.h): one block of an encoded.dat, from its headers."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("offset", "bytes", "reads", "records")] + \
               [("bad", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class PStats(ctypes.Structure):
    """ntc_p_stats (include/ntcomp_pipeline.h)."""
    _fields_ = [("pairs", ctypes.c_uint64), ("bytes1", ctypes.c_uint64), ("bytes2", ctypes.c_uint64),
                ("mode", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class DStats(ctypes.Structure):
    """ntc_d_stats (include/ntcomp_pipeline.h)."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("sections", "blocks_seq", "blocks_sym", "blocks_qual", "blocks_name")] + \
               [("not_checkable", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class NStats(ctypes.Structure):
    """ntc_n_stats (include/ntcomp_pipeline.h)."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("sections", "names", "name_bytes", "payload_bytes", "deflated_bytes")]


class BuildOpts(ctypes.Structure):
    """ntc_build_opts (include/ntcomp_host.h): memory bounds of the GPU index build."""
    _fields_ = [("device_budget_bytes", ctypes.c_uint64), ("host_budget_bytes", ctypes.c_uint64),
                ("temp_dir", ctypes.c_char_p), ("max_partition_keys", ctypes.c_uint64)]


class BuildStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("occurrences", "kmers", "sources", "nodes", "spilled_bytes",
                                               "device_budget_bytes", "pass_keys", "peak_device_bytes")] + \
               [(n, ctypes.c_uint32) for n in ("kmer_partitions", "node_partitions", "compactions", "seq_uploads")] + \
               [(n, ctypes.c_double) for n in ("seconds", "seconds_kmers", "seconds_sources", "seconds_nodes",
                                               "seconds_labels", "seconds_plan", "seconds_sort")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Timing(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_double), ("main_ms", ctypes.c_double), ("aux_ms", ctypes.c_double),
                ("units", ctypes.c_uint64), ("records", ctypes.c_uint64)]


_lib = None


def device_source_hash():
    """sha256 (16 hex) of the hot path's device code object -- the offload bundle of
    kernels.hip (k_pack, k_ms4, k_parse4, k_emit4, k_dec_rec, ...) inside the library's
    .hip_fatbin section: profiles/pmc_traffic.json records it, and bench.py uses counter data
    only when it matches the build it times.  Host-only or comment edits leave it unchanged."""
    import hashlib
    import struct
    with open(LIB_PATH, "rb") as f:
        b = f.read()
    shoff = struct.unpack_from("<Q", b, 0x28)[0]
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize) for i in range(shnum)]
    stro = secs[shstrndx][4]
    for sec in secs:
        name = b[stro + sec[0]:b.index(b"\0", stro + sec[0])]
        if name == b".hip_fatbin":
            fat = b[sec[4]:sec[4] + sec[5]]
            magic = b"__CLANG_OFFLOAD_BUNDLE__"
            parts = [magic + x for x in fat.split(magic)[1:]]
            hot = [x for x in parts if b"_ZN3ntc5k_ms4" in x]
            return hashlib.sha256(b"".join(hot or parts)).hexdigest()[:16]
    raise RuntimeError(f"{LIB_PATH}: no .hip_fatbin section")


def build_library(force=False):
    """Compile libntcomp_gpu.so in-tree for gfx950 (make -C ntcomp_amd/csrc)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(_HERE, "csrc")])
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} missing: build it with `make -C ntcomp_amd/csrc` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    P, u64, u32, i64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
    I = ctypes.c_int
    sig = {
        "ntc_abi_version": (I, []),
        "ntc_ctx_create": (I, [I, ctypes.POINTER(P)]),
        "ntc_ctx_destroy": (None, [P]),
        "ntc_last_error": (ctypes.c_char_p, [P]),
        "ntc_ctx_set_stream": (I, [P, P]),
        "ntc_ctx_synchronize": (I, [P]),
        "ntc_ctx_set_option": (I, [P, ctypes.c_char_p, i64]),
        "ntc_ctx_get_option": (I, [P, ctypes.c_char_p, ctypes.POINTER(i64)]),
        "ntc_index_upload": (I, [P, ctypes.POINTER(IndexView)]),
        "ntc_index_share": (I, [P, P]),
        "ntc_index_prepare": (I, [ctypes.POINTER(IndexView), ctypes.POINTER(P)]),
        "ntc_index_upload_prepared": (I, [P, P]),
        "ntc_index_prep_free": (None, [P]),
        "ntc_index_info": (I, [P, P, P, P]),
        "ntc_encode_batch": (I, [P, P, P, u64, P, u64, P, P]),
        "ntc_encode_batch_device": (I, [P, P, P, u64, u32, P, u64, P]),
        "ntc_encode_status": (I, [P, P, P]),
        "ntc_decode_batch": (I, [P, P, u64, P, u64, P, u64, P, P]),
        "ntc_decode_batch_device": (I, [P, P, u64, P, u64, P, u64]),
        "ntc_decode_status": (I, [P, P, P]),
        "ntc_last_timing": (I, [P, ctypes.POINTER(Timing)]),
        "ntc_device_alloc": (I, [P, u64, ctypes.POINTER(P)]),
        "ntc_device_free": (I, [P, P]),
        "ntc_memcpy_h2d": (I, [P, P, P, u64]),
        "ntc_memcpy_d2h": (I, [P, P, P, u64]),
        "ntc_debug_matching_statistics": (I, [P, P, P, u64, P, P]),
        "ntc_build_index": (I, [P, P, u64, u32, I, I, ctypes.POINTER(P)]),
        "ntc_build_index_device": (I, [P, P, P, u64, u32, I, ctypes.POINTER(P)]),
        "ntc_build_index_device_ex": (I, [P, P, P, u64, u32, I, ctypes.POINTER(BuildOpts),
                                          ctypes.POINTER(BuildStats), ctypes.POINTER(P)]),
        "ntc_index_set_prefix_precalc": (I, [P, u32]),
        "ntc_index_prefix_table": (I, [P, ctypes.POINTER(u32), P]),
        "ntc_index_free": (None, [P]),
        "ntc_index_view_of": (I, [P, ctypes.POINTER(IndexView)]),
        "ntc_index_save": (I, [P, ctypes.c_char_p]),
        "ntc_index_save_as": (I, [P, ctypes.c_char_p, I]),
        "ntc_index_load": (I, [ctypes.c_char_p, ctypes.POINTER(P)]),
        "ntc_synth_genome": (I, [u64, u64, P]),
        "ntc_synth_strains": (I, [P, u64, u64, u32, u32, P]),
        "ntc_minimizer_keys": (I, [P, u64, u32, u32, I, P]),
        "ntc_synth_reads": (I, [P, u64, u64, u64, u64, u32, u32, I, P]),
        "ntc_file_header": (None, [P]),
        "ntc_write_block": (I, [P, u64, u64, ctypes.POINTER(P), ctypes.POINTER(u64)]),
        "ntc_read_block": (I, [P, u64, ctypes.POINTER(u64), ctypes.POINTER(P), ctypes.POINTER(u64),
                               ctypes.POINTER(u64)]),
        "ntc_buffer_free": (None, [P]),
        "ntc_read_block_into": (I, [P, u64, ctypes.POINTER(u64), P, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "ntc_pack_block": (I, [P, u64, u64, ctypes.POINTER(BlockMeta), ctypes.POINTER(P), ctypes.POINTER(u64)]),
        "ntc_deflate_block": (I, [ctypes.POINTER(BlockMeta), P, I, ctypes.POINTER(P), ctypes.POINTER(u64)]),
        "ntc_deflate_stream": (I, [ctypes.POINTER(BlockMeta), I, P, I, ctypes.POINTER(P), ctypes.POINTER(u64)]),
        "ntc_pack_blocks_device": (I, [P, P, P, u64, u32, P, u64, P, ctypes.POINTER(u64)]),
        "ntc_deflate_blocks_device": (I, [P, P, P, u64, P, u64, P, ctypes.POINTER(u64)]),
        "ntc_encode_members": (I, [P, P, u64, ctypes.POINTER(u64)]),
        "ntc_inflate_members": (I, [P, P, u64, P, u64, P, u64, P, ctypes.POINTER(u64)]),
        "ntc_inflate_members_device": (I, [P, P, u64, P, u64, P, u64, P, ctypes.POINTER(u64)]),
        "ntc_bgzf_bound": (u64, [u64]),
        "ntc_bgzf_compress": (I, [P, P, u64, P, u64, P, u64, P, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "ntc_bgzf_compress_device": (I, [P, P, u64, P, u64, P, u64, P, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "ntc_bgzf_last": (I, [P, P, P, u64, ctypes.POINTER(u64)]),
        "ntc_encode_pack_batch": (I, [P, P, P, u64, u32, P, ctypes.POINTER(P), ctypes.POINTER(u64),
                                      ctypes.POINTER(i64)]),
        "ntc_fastq_parse": (I, [P, P, u64, u64, P, u64, P, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_int64)]),
        "ntc_encode_pack_fastq": (I, [P, P, u64, u64, u32, P, ctypes.POINTER(P), ctypes.POINTER(u64),
                                      ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_int64)]),
        "ntc_encode_pack_fastq_paired": (I, [P, P, u64, P, u64, u64, u32, P, ctypes.POINTER(P), ctypes.POINTER(u64),
                                             ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_int64)]),
        "ntc_decode_pair_split": (I, [P, ctypes.POINTER(u64)]),
        "ntc_fastx_open": (I, [ctypes.c_char_p, ctypes.POINTER(P)]),
        "ntc_fastx_next_batch": (I, [P, u64, u64, ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(u64)]),
        "ntc_fastx_close": (None, [P]),
        "ntc_fastx_next_batch_into": (I, [P, u64, u64, P, u64, P, ctypes.POINTER(u64)]),
        "ntc_fastx_set_threads": (I, [P, I]),
        "ntc_host_threads": (I, []),
        "ntc_encode_file": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(PipelineOpts), ctypes.POINTER(PipelineStats)]),
        "ntc_fasta_format": (I, [P, P, u64, u64, ctypes.POINTER(P), ctypes.POINTER(u64)]),
        "ntc_decode_fasta": (I, [P, P, u64, u64, u64, u64, P, u64, ctypes.POINTER(u64)]),
        "ntc_decode_file": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(PipelineOpts), ctypes.POINTER(PipelineStats)]),
        "ntc_read_block_streams": (I, [P, u64, ctypes.POINTER(u64), P, u64, ctypes.POINTER(BlockMeta)]),
        "ntc_unpack_streams": (I, [P, P, u64, P, u64, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "ntc_unpacked_records": (I, [P, P, u64, ctypes.POINTER(u64)]),
        "ntc_decode_fasta_unpacked": (I, [P, u64, P, u64, ctypes.POINTER(u64)]),
        "ntc_encode_exceptions": (I, [P, P, u64, ctypes.POINTER(u64)]),
        "ntc_decode_set_exceptions": (I, [P, P, u64, u32]),
        "ntc_encode_qualities": (I, [P, P, u64, P, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "ntc_decode_set_qualities": (I, [P, P, u64, P, u64]),
        "ntc_q_write_header": (I, [I, I]),
        "ntc_q_write_header2": (I, [I, I, I]),
        "ntc_q_deflate_section": (I, [P, P, I, ctypes.POINTER(P), ctypes.POINTER(u64)]),
        "ntc_q_write_section": (I, [I, P, P, I]),
        "ntc_q_read": (I, [ctypes.c_char_p, ctypes.POINTER(I), ctypes.POINTER(P), ctypes.POINTER(u64),
                           ctypes.POINTER(P), ctypes.POINTER(u64)]),
        "ntc_encode_names": (I, [P, P, u64, P, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "ntc_decode_set_names": (I, [P, P, u64, P, u64]),
        "ntc_n_write_header": (I, [I, I]),
        "ntc_n_deflate_section": (I, [P, P, I, ctypes.POINTER(P), ctypes.POINTER(u64)]),
        "ntc_n_write_section": (I, [I, P, P, I]),
        "ntc_n_read": (I, [ctypes.c_char_p, ctypes.POINTER(I), ctypes.POINTER(P), ctypes.POINTER(u64),
                           ctypes.POINTER(P), ctypes.POINTER(u64)]),
        "ntc_encode_digests": (I, [P, P, u64, ctypes.POINTER(u64)]),
        "ntc_decode_set_digests": (I, [P, P, u64]),
        "ntc_decode_digests": (I, [P, P, u64, ctypes.POINTER(u64)]),
        "ntc_d_write_header": (I, [I, u32, u32, u64]),
        "ntc_d_write_section": (I, [I, P]),
        "ntc_d_read": (I, [ctypes.c_char_p, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u64),
                           ctypes.POINTER(P), ctypes.POINTER(u64)]),
        "ntc_encode_file_ex2": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(FileOpts2), ctypes.POINTER(PipelineOpts),
                                    ctypes.POINTER(PipelineStats), ctypes.POINTER(NxStats), ctypes.POINTER(QStats),
                                    ctypes.POINTER(NStats)]),
        "ntc_decode_file_ex2": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(FileOpts2), ctypes.POINTER(PipelineOpts),
                                    ctypes.POINTER(PipelineStats)]),
        "ntc_encode_file_ex6": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(FileOpts6), ctypes.POINTER(PipelineOpts),
                                    ctypes.POINTER(PipelineStats), ctypes.POINTER(NxStats), ctypes.POINTER(QStats),
                                    ctypes.POINTER(NStats), ctypes.POINTER(DStats), ctypes.POINTER(PStats),
                                    ctypes.POINTER(IStats)]),
        "ntc_encode_file_ex3": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(FileOpts3), ctypes.POINTER(PipelineOpts),
                                    ctypes.POINTER(PipelineStats), ctypes.POINTER(NxStats), ctypes.POINTER(QStats),
                                    ctypes.POINTER(NStats), ctypes.POINTER(DStats)]),
        "ntc_encode_file_ex4": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(FileOpts4), ctypes.POINTER(PipelineOpts),
                                    ctypes.POINTER(PipelineStats), ctypes.POINTER(NxStats), ctypes.POINTER(QStats),
                                    ctypes.POINTER(NStats), ctypes.POINTER(DStats), ctypes.POINTER(PStats)]),
        "ntc_decode_file_ex4": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(FileOpts4), ctypes.POINTER(PipelineOpts),
                                    ctypes.POINTER(PipelineStats), ctypes.POINTER(DStats), ctypes.POINTER(PStats)]),
        "ntc_decode_file_ex3": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(FileOpts3), ctypes.POINTER(PipelineOpts),
                                    ctypes.POINTER(PipelineStats), ctypes.POINTER(DStats)]),
        "ntc_decode_file_ex5": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(FileOpts5), ctypes.POINTER(PipelineOpts),
                                    ctypes.POINTER(PipelineStats), ctypes.POINTER(DStats), ctypes.POINTER(PStats),
                                    ctypes.POINTER(RStats)]),
        "ntc_decode_file_ex7": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(FileOpts7), ctypes.POINTER(PipelineOpts),
                                    ctypes.POINTER(PipelineStats), ctypes.POINTER(DStats), ctypes.POINTER(PStats),
                                    ctypes.POINTER(RStats), ctypes.POINTER(ZStats)]),
        "ntc_decode_set_window": (I, [P, u64, u64]),
        "ntc_archive_info": (I, [ctypes.c_char_p, ctypes.POINTER(P), ctypes.POINTER(u64), ctypes.POINTER(u64),
                                 ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "ntc_nx_write": (I, [I, P, u64, u32, I]),
        "ntc_nx_read": (I, [ctypes.c_char_p, ctypes.POINTER(P), ctypes.POINTER(u64), ctypes.POINTER(u32)]),
        "ntc_encode_file_nx": (I, [P, I, ctypes.c_char_p, I, I, I, ctypes.POINTER(PipelineOpts),
                                   ctypes.POINTER(PipelineStats), ctypes.POINTER(NxStats)]),
        "ntc_encode_file_ex": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(FileOpts), ctypes.POINTER(PipelineOpts),
                                   ctypes.POINTER(PipelineStats), ctypes.POINTER(NxStats), ctypes.POINTER(QStats)]),
        "ntc_decode_file_ex": (I, [P, I, ctypes.c_char_p, I, ctypes.POINTER(FileOpts), ctypes.POINTER(PipelineOpts),
                                   ctypes.POINTER(PipelineStats)]),
        "ntc_decode_file_nx": (I, [P, I, ctypes.c_char_p, ctypes.c_char_p, I, ctypes.POINTER(PipelineOpts),
                                   ctypes.POINTER(PipelineStats)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def pack_reads(reads):
    """list[bytes|str] -> (uint8 bases, uint64 offsets[n+1])."""
    bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    offs = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8)[: int(offs[-1])].copy(), offs


class Index:
    """Host SBWT subset matrix + LCS (ntc_index_host)."""

    def __init__(self, handle):
        self.h = handle
        self._view = IndexView()
        rc = lib().ntc_index_view_of(self.h, ctypes.byref(self._view))
        if rc:
            raise NtcError(rc, "index view")

    @classmethod
    def build(cls, seqs, k, add_revcomp=True, threads=0):
        bases, offs = pack_reads(seqs)
        h = ctypes.c_void_p()
        rc = lib().ntc_build_index(_p(bases), _p(offs), len(offs) - 1, k, int(add_revcomp), threads,
                                   ctypes.byref(h))
        if rc:
            raise NtcError(rc, "ntc_build_index")
        return cls(h)

    @classmethod
    def build_gpu(cls, ctx, seqs, k, add_revcomp=True, device_budget=0, host_budget=0, temp_dir=None,
                  max_partition_keys=0, stats=None):
        """The same index built on ctx's GPU (ntc_build_index_device_ex, build.hip), in
        passes that fit device_budget bytes (0: 85 % of free HBM), sorted partitions held on
        the host up to host_budget bytes (0: no limit), past it in files under temp_dir.
        seqs: list of bytes/str, or a (bases uint8, offsets uint64[n+1]) pair.  stats: a dict
        filled with ntc_build_stats."""
        if isinstance(seqs, tuple) and len(seqs) == 2 and isinstance(seqs[0], np.ndarray):
            bases, offs = np.ascontiguousarray(seqs[0], np.uint8), np.ascontiguousarray(seqs[1], np.uint64)
        else:
            bases, offs = pack_reads(seqs)
        h = ctypes.c_void_p()
        o = BuildOpts(device_budget, host_budget, str(temp_dir).encode() if temp_dir else None, max_partition_keys)
        st = BuildStats()
        rc = lib().ntc_build_index_device_ex(ctx.h, _p(bases), _p(offs), len(offs) - 1, k, int(add_revcomp),
                                             ctypes.byref(o), ctypes.byref(st), ctypes.byref(h))
        if stats is not None:
            stats.update(st.as_dict())
        if rc:
            raise NtcError(rc, lib().ntc_last_error(ctx.h).decode(errors="replace"))
        return cls(h)

    def set_prefix_precalc(self, p):
        """-p/--prefix-precalc: the colex interval of every p-mer (sbwt's PrefixLookupTable),
        written with the sbwt-rs layout."""
        rc = lib().ntc_index_set_prefix_precalc(self.h, p)
        if rc:
            raise NtcError(rc, f"ntc_index_set_prefix_precalc({p})")

    def prefix_table(self):
        """(p, ranges uint64[4^p, 2]) or (0, None)."""
        p = ctypes.c_uint32()
        lib().ntc_index_prefix_table(self.h, ctypes.byref(p), None)
        if not p.value:
            return 0, None
        r = np.zeros((4 ** p.value, 2), dtype=np.uint64)
        lib().ntc_index_prefix_table(self.h, ctypes.byref(p), _p(r))
        return p.value, r

    @classmethod
    def load(cls, prefix):
        h = ctypes.c_void_p()
        rc = lib().ntc_index_load(str(prefix).encode(), ctypes.byref(h))
        if rc:
            raise NtcError(rc, f"ntc_index_load({prefix})")
        return cls(h)

    def save(self, prefix, layout="own"):
        """layout "own" (default) or "sbwt-rs" (a recalled restatement of sbwt 0.3.11 / kbo
        0.5.1 files, parity unpinned); Index.load detects either."""
        code = {"own": 0, "sbwt-rs": 1}[layout]
        rc = lib().ntc_index_save_as(self.h, str(prefix).encode(), code)
        if rc:
            raise NtcError(rc, f"ntc_index_save_as({prefix}, {layout})")

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.ntc_index_free(self.h)
            self.h = None

    @property
    def view(self):
        return self._view

    @property
    def n(self):
        return int(self._view.n_nodes)

    @property
    def k(self):
        return int(self._view.k)

    @property
    def C(self):
        return [int(x) for x in self._view.C]

    def row(self, c):
        words = (self.n + 63) // 64
        buf = (ctypes.c_uint64 * words).from_address(self._view.rows[c])
        return np.frombuffer(buf, dtype=np.uint64).copy()

    @property
    def rows(self):
        return [self.row(c) for c in range(4)]

    @property
    def lcs(self):
        buf = (ctypes.c_uint8 * self.n).from_address(self._view.lcs)
        return np.frombuffer(buf, dtype=np.uint8).copy()


class GpuContext:
    """One HIP context (device + stream + resident index) of libntcomp_gpu.so."""

    def __init__(self, device=0):
        self.L = lib()
        self.h = ctypes.c_void_p()
        rc = self.L.ntc_ctx_create(device, ctypes.byref(self.h))
        if rc:
            raise NtcError(rc, f"ntc_ctx_create({device}): no usable GPU")
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.L.ntc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc:
            raise NtcError(rc, f"{what}: {self.L.ntc_last_error(self.h).decode(errors='replace')}")

    def upload(self, index):
        self._check(self.L.ntc_index_upload(self.h, ctypes.byref(index.view)), "ntc_index_upload")
        return self

    def upload_prepared(self, prep):
        """Upload an IndexPrep (ntc_index_prepare's host tables, built once for any number of
        contexts / devices): ntc_index_upload_prepared."""
        self._check(self.L.ntc_index_upload_prepared(self.h, prep.h), "ntc_index_upload_prepared")
        return self

    def share_index(self, other):
        """Use other's device index (same GPU, ntc_index_share): no second upload or copy."""
        self._check(self.L.ntc_index_share(self.h, other.h), "ntc_index_share")
        return self

    def upload_arrays(self, n, k, rows, C, lcs):
        rows = [np.ascontiguousarray(r, dtype=np.uint64) for r in rows]
        lcs = np.ascontiguousarray(lcs, dtype=np.uint8)
        v = IndexView()
        v.n_nodes, v.k = int(n), int(k)
        for c in range(4):
            v.rows[c] = rows[c].ctypes.data
            v.C[c] = int(C[c])
        v.lcs = lcs.ctypes.data
        self._check(self.L.ntc_index_upload(self.h, ctypes.byref(v)), "ntc_index_upload")
        return self

    def set_option(self, key, value):
        self._check(self.L.ntc_ctx_set_option(self.h, key.encode(), int(value)), f"set_option({key})")

    def get_option(self, key):
        v = ctypes.c_int64()
        self._check(self.L.ntc_ctx_get_option(self.h, key.encode(), ctypes.byref(v)), f"get_option({key})")
        return int(v.value)

    def index_info(self):
        n, k, b = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint64()
        self._check(self.L.ntc_index_info(self.h, ctypes.byref(n), ctypes.byref(k), ctypes.byref(b)), "info")
        return int(n.value), int(k.value), int(b.value)

    # ---- non-ACGT symbols ----------------------------------------------------------
    class _Policy:
        """`with ctx._policy(p)`: the context's "non_acgt" option is p inside (None: left alone)."""

        def __init__(self, ctx, non_acgt):
            self.ctx, self.new = ctx, None if non_acgt is None else _policy_code(non_acgt)

        def __enter__(self):
            if self.new is not None:
                self.old = self.ctx.get_option("non_acgt")
                self.ctx.set_option("non_acgt", self.new)

        def __exit__(self, *exc):
            if self.new is not None:
                self.ctx.set_option("non_acgt", self.old)

    def _policy(self, non_acgt):
        return GpuContext._Policy(self, non_acgt)

    # ---- quality scores -------------------------------------------------------------
    class _Option:
        """`with ctx._option(key, v)`: the context's option is v inside (None: left alone)."""

        def __init__(self, ctx, key, value):
            self.ctx, self.key, self.new = ctx, key, value

        def __enter__(self):
            if self.new is not None:
                self.old = self.ctx.get_option(self.key)
                self.ctx.set_option(self.key, self.new)

        def __exit__(self, *exc):
            if self.new is not None:
                self.ctx.set_option(self.key, self.old)

    def _qmode(self, qualities):
        return GpuContext._Option(self, "qualities", None if qualities is None else _quality_code(qualities))

    def _qcoder(self, coder):
        return GpuContext._Option(self, "quality_coder", None if coder is None else _coder_code(coder))

    @property
    def quality_coder(self):
        """The coder of the quality sections encode_pack_fastq makes ("quality_coder"): 0 pack, 1 rans."""
        return self.get_option("quality_coder")

    @quality_coder.setter
    def quality_coder(self, coder):
        self.set_option("quality_coder", _coder_code(coder))

    def _qsmooth(self, m):
        return GpuContext._Option(self, "quality_smooth", None if m is None else _smooth_code(m))

    def _qsmooth_to(self, to):
        return GpuContext._Option(self, "quality_smooth_to", None if to is None else _smooth_to_code(to))

    @property
    def quality_smooth(self):
        """Smoothing inside long matches ("quality_smooth"): 0 off, or M: a quality above the mode's image of
        '#' that lies in a long record of at least M bases becomes quality_smooth_to."""
        return self.get_option("quality_smooth")

    @quality_smooth.setter
    def quality_smooth(self, m):
        self.set_option("quality_smooth", _smooth_code(m))

    @property
    def quality_smooth_to(self):
        """The byte smoothing writes ("quality_smooth_to"), as bytes of length 1."""
        return bytes([self.get_option("quality_smooth_to")])

    @quality_smooth_to.setter
    def quality_smooth_to(self, to):
        self.set_option("quality_smooth_to", _smooth_to_code(to))

    @property
    def quality_smoothed(self):
        """Quality bytes the last encode_pack_fastq call replaced ("quality_smoothed", read-only)."""
        return self.get_option("quality_smoothed")

    def qualities(self):
        """The quality sections of the last encode_pack_fastq call under "keep" or "bin8"
        (ntc_encode_qualities) -> (list of QualMeta, their packed words as bytes)."""
        nb, nbytes = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.L.ntc_encode_qualities(self.h, None, 0, None, 0, ctypes.byref(nb), ctypes.byref(nbytes))
        if rc not in (0, 5):
            self._check(rc, "ntc_encode_qualities")
        metas = (QualMeta * max(nb.value, 1))()
        pay = np.zeros(max(nbytes.value, 8), dtype=np.uint8)
        if nb.value:
            self._check(self.L.ntc_encode_qualities(self.h, metas, nb.value, _p(pay), len(pay), ctypes.byref(nb),
                                                    ctypes.byref(nbytes)), "ntc_encode_qualities")
        return list(metas)[:nb.value], pay[:nbytes.value].tobytes()

    def set_qualities(self, metas, payload):
        """Quality sections (QualMeta, in read order) for the next decode_fasta /
        decode_fasta_unpacked call, which then returns FASTQ (ntc_decode_set_qualities)."""
        arr = (QualMeta * max(len(metas), 1))(*metas)
        buf = np.frombuffer(bytes(payload), dtype=np.uint8) if len(payload) else np.zeros(8, dtype=np.uint8)
        self._check(self.L.ntc_decode_set_qualities(self.h, arr, len(metas), _p(buf), len(payload)),
                    "ntc_decode_set_qualities")

    # ---- read names ------------------------------------------------------------------
    def _nmode(self, names):
        return GpuContext._Option(self, "names", None if names is None else _names_code(names))

    def names(self):
        """The name sections of the last encode_pack_fastq call under "keep" or "id"
        (ntc_encode_names) -> (list of NameMeta, their payload as bytes)."""
        nb, nbytes = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.L.ntc_encode_names(self.h, None, 0, None, 0, ctypes.byref(nb), ctypes.byref(nbytes))
        if rc not in (0, 5):
            self._check(rc, "ntc_encode_names")
        metas = (NameMeta * max(nb.value, 1))()
        pay = np.zeros(max(nbytes.value, 8), dtype=np.uint8)
        if nb.value:
            self._check(self.L.ntc_encode_names(self.h, metas, nb.value, _p(pay), len(pay), ctypes.byref(nb),
                                                ctypes.byref(nbytes)), "ntc_encode_names")
        return list(metas)[:nb.value], pay[:nbytes.value].tobytes()

    def set_names(self, metas, payload):
        """Name sections (NameMeta, in read order) for the next decode_fasta /
        decode_fasta_unpacked call, which then prints the names (ntc_decode_set_names)."""
        arr = (NameMeta * max(len(metas), 1))(*metas)
        buf = np.frombuffer(bytes(payload), dtype=np.uint8) if len(payload) else np.zeros(8, dtype=np.uint8)
        self._check(self.L.ntc_decode_set_names(self.h, arr, len(metas), _p(buf), len(payload)),
                    "ntc_decode_set_names")

    # ---- content digests ---------------------------------------------------------------
    @property
    def digests(self):
        """Option "digests": 1 makes encode_pack and encode_pack_fastq digest every block on the GPU."""
        return self.get_option("digests")

    @digests.setter
    def digests(self, on):
        self.set_option("digests", 1 if on else 0)

    def _digests(self, digests):
        return GpuContext._Option(self, "digests", None if digests is None else (1 if digests else 0))

    def _digest_table(self, fn, what):
        nb = ctypes.c_uint64()
        rc = fn(self.h, None, 0, ctypes.byref(nb))
        if rc not in (0, 5):
            self._check(rc, what)
        metas = (DigestMeta * max(nb.value, 1))()
        if nb.value:
            self._check(fn(self.h, metas, nb.value, ctypes.byref(nb)), what)
        return list(metas)[:nb.value]

    def encode_digests(self):
        """The digests of the last encode_pack / encode_pack_fastq call with digests on
        (ntc_encode_digests) -> list of DigestMeta, one per block."""
        return self._digest_table(self.L.ntc_encode_digests, "ntc_encode_digests")

    def decode_set_digests(self, metas):
        """Expected digests (DigestMeta, in read order) for the next decode_fasta_unpacked call, which
        then checks what it decoded against them on the GPU (ntc_decode_set_digests)."""
        arr = (DigestMeta * max(len(metas), 1))(*metas)
        self._check(self.L.ntc_decode_set_digests(self.h, arr, len(metas)), "ntc_decode_set_digests")

    def decode_digests(self):
        """What the last decode call that was given expected digests computed, also after
        NTC_ERR_DIGEST (ntc_decode_digests); components says which were checked."""
        return self._digest_table(self.L.ntc_decode_digests, "ntc_decode_digests")

    def exceptions(self):
        """The exception runs of the last encode / encode_pack / encode_pack_fastq call under
        policy keep (ntc_encode_exceptions), as a structured array of dtype NX_RUN in (read,
        pos) order."""
        n = ctypes.c_uint64()
        rc = self.L.ntc_encode_exceptions(self.h, None, 0, ctypes.byref(n))
        if rc not in (0, 5):
            self._check(rc, "ntc_encode_exceptions")
        runs = np.zeros(n.value, dtype=NX_RUN)
        if n.value:
            self._check(self.L.ntc_encode_exceptions(self.h, _p(runs), len(runs), ctypes.byref(n)),
                        "ntc_encode_exceptions")
        return runs

    def set_exceptions(self, runs, sub):
        """Exception runs (dtype NX_RUN, read relative to the next call's first read) and the
        substitute base for the next decode / decode_fasta call (ntc_decode_set_exceptions)."""
        runs = np.ascontiguousarray(runs, dtype=NX_RUN)
        sub = sub if isinstance(sub, int) else ord(sub)
        self._check(self.L.ntc_decode_set_exceptions(self.h, _p(runs) if len(runs) else None, len(runs), sub),
                    "ntc_decode_set_exceptions")

    @property
    def substitute(self):
        """The substitute base of the uploaded index (option "nx_sub"), as an int."""
        return self.get_option("nx_sub")

    # ---- encode ------------------------------------------------------------------
    def encode(self, bases, offsets, non_acgt=None):
        """-> (uint64 records, uint64 rec_offsets[n_reads+1]); raises NtcError(code) with
        .bad_read on a failing read.  non_acgt ("error", "mask" or "keep"; None leaves the
        context's option alone): the call runs under that policy and returns (records,
        rec_offsets, exception runs)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nreads = len(offsets) - 1
        total = int(offsets[-1] - offsets[0]) if nreads >= 0 else 0
        recs = np.zeros(total + 1, dtype=np.uint64)
        roff = np.zeros(nreads + 1, dtype=np.uint64)
        bad = ctypes.c_int64(-1)
        with self._policy(non_acgt):
            rc = self.L.ntc_encode_batch(self.h, _p(bases), _p(offsets), nreads, _p(recs), len(recs), _p(roff),
                                         ctypes.byref(bad))
        if rc:
            e = NtcError(rc, self.L.ntc_last_error(self.h).decode(errors="replace"))
            e.bad_read = bad.value
            raise e
        if non_acgt is not None:
            return recs[: int(roff[-1])], roff, self.exceptions()
        return recs[: int(roff[-1])], roff

    def decode(self, recs):
        recs = np.ascontiguousarray(recs, dtype=np.uint64)
        nr, nb = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.L.ntc_decode_batch(self.h, _p(recs), len(recs), None, 0, None, 0, ctypes.byref(nr),
                                     ctypes.byref(nb))
        if rc not in (0, 5):
            self._check(rc, "ntc_decode_batch")
        out = np.zeros(int(nb.value) + 1, dtype=np.uint8)
        offs = np.zeros(int(nr.value) + 1, dtype=np.uint64)
        self._check(self.L.ntc_decode_batch(self.h, _p(recs), len(recs), _p(out), len(out), _p(offs), len(offs),
                                            ctypes.byref(nr), ctypes.byref(nb)), "ntc_decode_batch")
        return out[: int(nb.value)], offs

    def matching_statistics(self, bases, offsets):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        total = int(offsets[-1] - offsets[0])
        d = np.zeros(total + 1, dtype=np.uint32)
        s = np.zeros(total + 1, dtype=np.uint32)
        self._check(self.L.ntc_debug_matching_statistics(self.h, _p(bases), _p(offsets), len(offsets) - 1,
                                                         _p(d), _p(s)), "ntc_debug_matching_statistics")
        return d[:total], s[:total]

    # ---- device-resident buffers (bench) ---------------------------------------------
    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._check(self.L.ntc_device_alloc(self.h, int(nbytes), ctypes.byref(p)), "ntc_device_alloc")
        return p.value

    def free(self, ptr):
        self._check(self.L.ntc_device_free(self.h, ctypes.c_void_p(ptr)), "ntc_device_free")

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._check(self.L.ntc_memcpy_h2d(self.h, ctypes.c_void_p(dptr), _p(arr), arr.nbytes), "h2d")

    def d2h(self, arr, dptr):
        self._check(self.L.ntc_memcpy_d2h(self.h, _p(arr), ctypes.c_void_p(dptr), arr.nbytes), "d2h")
        return arr

    def encode_device(self, d_bases, d_offs, n_reads, max_read_len, d_recs, cap, d_roffs):
        self._check(self.L.ntc_encode_batch_device(self.h, ctypes.c_void_p(d_bases), ctypes.c_void_p(d_offs),
                                                   n_reads, max_read_len, ctypes.c_void_p(d_recs), cap,
                                                   ctypes.c_void_p(d_roffs)), "ntc_encode_batch_device")

    def pack_device(self, d_recs, d_roffs, n_reads, block_reads, d_payload, cap):
        """GPU packer (ntc_pack_blocks_device) -> (list of BlockMeta, payload bytes used)."""
        nb = (n_reads + block_reads - 1) // block_reads
        metas = (BlockMeta * max(nb, 1))()
        used = ctypes.c_uint64()
        self._check(self.L.ntc_pack_blocks_device(self.h, ctypes.c_void_p(d_recs), ctypes.c_void_p(d_roffs), n_reads,
                                                  block_reads, ctypes.c_void_p(d_payload), cap, metas,
                                                  ctypes.byref(used)), "ntc_pack_blocks_device")
        return list(metas)[:nb], int(used.value)

    def deflate_device(self, d_payload, metas, d_out, cap):
        """The gzip members of packed blocks, made on the GPU (ntc_deflate_blocks_device): d_payload
        and metas as pack_device left them -> (uint64 array [blocks, 4, 2] of each member's offset in
        d_out and its bytes, bytes used).  NtcError(NTC_ERR_CAPACITY) carries .needed."""
        arr = (BlockMeta * max(len(metas), 1))(*metas)
        off_len = np.zeros((len(metas), 4, 2), dtype=np.uint64)
        used = ctypes.c_uint64()
        rc = self.L.ntc_deflate_blocks_device(self.h, ctypes.c_void_p(d_payload), arr, len(metas), ctypes.c_void_p(d_out),
                                              cap, _p(off_len) if len(metas) else None, ctypes.byref(used))
        if rc:
            e = NtcError(rc, self.L.ntc_last_error(self.h).decode(errors="replace"))
            e.needed = int(used.value)
            raise e
        return off_len, int(used.value)

    def inflate_members_device(self, d_comp, comp_bytes, members, d_dst, dst_cap):
        """Inflate gzip members from one device buffer into another (ntc_inflate_members_device):
        members as for inflate_members -> an INFLATE_RESULT array."""
        m = _inflate_descs(members)
        res = np.zeros(len(m), dtype=INFLATE_RESULT)
        bad = ctypes.c_uint64()
        self._check(self.L.ntc_inflate_members_device(self.h, ctypes.c_void_p(d_comp), comp_bytes, _p(m) if len(m) else None,
                                                      len(m), ctypes.c_void_p(d_dst), dst_cap,
                                                      _p(res) if len(m) else None, ctypes.byref(bad)),
                    "ntc_inflate_members_device")
        return res

    def bgzf_compress_device(self, d_text, n, d_out, cap, d_rec_off=0, n_rec=0):
        """The BGZF members of the n bytes at d_text, made on the GPU into d_out
        (ntc_bgzf_compress_device); d_rec_off (0: plain cuts): n_rec + 1 uint64 record offsets on the
        device -> (a BGZF_MEMBER array, bytes used).  NtcError(NTC_ERR_CAPACITY) carries .needed."""
        tab = np.zeros(max(1, bgzf_members_max(n)), dtype=BGZF_MEMBER)
        nm, used = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.L.ntc_bgzf_compress_device(self.h, ctypes.c_void_p(d_text), n, ctypes.c_void_p(d_rec_off) if d_rec_off else None,
                                             n_rec, ctypes.c_void_p(d_out), cap, _p(tab), len(tab), ctypes.byref(nm),
                                             ctypes.byref(used))
        if rc:
            e = NtcError(rc, self.L.ntc_last_error(self.h).decode(errors="replace"))
            e.needed = int(used.value)
            raise e
        return tab[:nm.value].copy(), int(used.value)

    @property
    def bgzf_text(self):
        """Whether the text decode calls leave BGZF members in place of their text (ctx option "bgzf_text")."""
        return bool(self.get_option("bgzf_text"))

    @bgzf_text.setter
    def bgzf_text(self, on):
        self.set_option("bgzf_text", 1 if on else 0)

    def bgzf_last(self):
        """What the last call that made BGZF members left (ntc_bgzf_last): bgzf_compress with this
        context, bgzf_compress_device, or a text decode under bgzf_text -> (dict of members, text_bytes,
        bytes, chunks_stored, chunks_huffman, chunks_matches; a BGZF_MEMBER array)."""
        c = np.zeros(7, dtype=np.uint64)  # ntc_bgzf_counts: six counts, then the seconds as a double
        nm = ctypes.c_uint64()
        self._check(self.L.ntc_bgzf_last(self.h, _p(c), None, 0, ctypes.byref(nm)), "ntc_bgzf_last")
        tab = np.zeros(max(1, nm.value), dtype=BGZF_MEMBER)
        self._check(self.L.ntc_bgzf_last(self.h, _p(c), _p(tab), len(tab), ctypes.byref(nm)), "ntc_bgzf_last")
        keys = ("members", "text_bytes", "bytes", "chunks_stored", "chunks_huffman", "chunks_matches")
        counts = dict(zip(keys, (int(v) for v in c[:6])))
        counts["seconds"] = float(c[6:].view(np.float64)[0])
        return counts, tab[:nm.value].copy()

    def encode_members(self):
        """Where the members lie in the payload of the last encode_pack* call under option
        "gpu_deflate" (ntc_encode_members) -> uint64 array [blocks, 4, 2] of (offset, bytes)."""
        nb = ctypes.c_uint64()
        rc = self.L.ntc_encode_members(self.h, None, 0, ctypes.byref(nb))
        if rc not in (0, 5):
            self._check(rc, "ntc_encode_members")
        off_len = np.zeros((nb.value, 4, 2), dtype=np.uint64)
        if nb.value:
            self._check(self.L.ntc_encode_members(self.h, _p(off_len), nb.value, ctypes.byref(nb)), "ntc_encode_members")
        return off_len

    def encode_pack(self, bases, offsets, block_reads=65536, non_acgt=None, digests=None):
        """Reads -> packed blocks (ntc_encode_pack_batch): the records stay in HBM and the
        GPU packer writes each block's four streams; returns (list of BlockMeta, payload
        bytes) ready for deflate_block.  With non_acgt (as for encode) the exception runs
        come third.  With digests (True / False; the call runs under it) the blocks' DigestMeta
        come last, as encode_digests() returns them."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nreads = len(offsets) - 1
        nb = (nreads + block_reads - 1) // block_reads
        metas = (BlockMeta * max(nb, 1))()
        out, used, bad = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int64(-1)
        b = bases if len(bases) else np.zeros(1, dtype=np.uint8)
        with self._policy(non_acgt), self._digests(digests):
            rc = self.L.ntc_encode_pack_batch(self.h, _p(b), _p(offsets), nreads, block_reads, metas,
                                              ctypes.byref(out), ctypes.byref(used), ctypes.byref(bad))
        if rc:
            e = NtcError(rc, self.L.ntc_last_error(self.h).decode(errors="replace"))
            e.bad_read = bad.value
            raise e
        try:
            payload = ctypes.string_at(out.value, used.value) if used.value else b""
        finally:
            self.L.ntc_buffer_free(out)
        out = (list(metas)[:nb], payload)
        if non_acgt is not None:
            out += (self.exceptions(),)
        if digests is not None:
            out += (self.encode_digests(),)
        return out

    def parse_fastq(self, text, n_reads):
        """Plain FASTQ text of exactly n_reads 4-line records -> (bases, offsets), parsed on
        the GPU (ntc_fastq_parse, fastq.hip); NtcError(NTC_ERR_FORMAT) with .bad_read."""
        t = np.frombuffer(bytes(text), dtype=np.uint8) if len(text) else np.zeros(1, dtype=np.uint8)
        bases = np.empty(len(text) // 2 + 1, dtype=np.uint8)
        offs = np.zeros(n_reads + 1, dtype=np.uint64)
        nb, bad = ctypes.c_uint64(), ctypes.c_int64(-1)
        rc = self.L.ntc_fastq_parse(self.h, _p(t), len(text), n_reads, _p(bases), len(bases), _p(offs),
                                    ctypes.byref(nb), ctypes.byref(bad))
        if rc:
            e = NtcError(rc, self.L.ntc_last_error(self.h).decode(errors="replace"))
            e.bad_read = bad.value
            raise e
        return bases[:nb.value].copy(), offs

    def encode_pack_fastq(self, text, n_reads, block_reads=65536, non_acgt=None, qualities=None, names=None,
                          quality_coder=None, digests=None, quality_smooth=None, quality_smooth_to=None):
        """encode_pack on FASTQ text parsed on the GPU (ntc_encode_pack_fastq) -> (list of
        BlockMeta, payload bytes, bases encoded).  With non_acgt (as for encode) the exception
        runs come fourth.  With qualities ("drop", "keep" or "bin8"; the call runs under that
        mode) the quality sections come next, as qualities() returns them, and with names ("drop",
        "keep" or "id") the name sections come last, as names() returns them.  quality_coder ("pack" or
        "rans"; the call runs under it): the coder of the quality sections.  With digests (True / False;
        the call runs under it) the blocks' DigestMeta come after all of those, as encode_digests()
        returns them.  quality_smooth (0 or M) and quality_smooth_to (one byte) hold for the call
        only, as quality_coder does: the qualities inside long records of at least M bases become
        that byte before they are coded."""
        t = np.frombuffer(bytes(text), dtype=np.uint8) if len(text) else np.zeros(1, dtype=np.uint8)
        nb = (n_reads + block_reads - 1) // block_reads
        metas = (BlockMeta * max(nb, 1))()
        out, used, nbases, bad = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int64(-1)
        with self._policy(non_acgt), self._qmode(qualities), self._nmode(names), self._qcoder(quality_coder), \
                self._digests(digests), self._qsmooth(quality_smooth), self._qsmooth_to(quality_smooth_to):
            rc = self.L.ntc_encode_pack_fastq(self.h, _p(t), len(text), n_reads, block_reads, metas,
                                              ctypes.byref(out), ctypes.byref(used), ctypes.byref(nbases),
                                              ctypes.byref(bad))
        if rc:
            self.L.ntc_buffer_free(out)
            e = NtcError(rc, self.L.ntc_last_error(self.h).decode(errors="replace"))
            e.bad_read = bad.value
            raise e
        try:
            payload = ctypes.string_at(out.value, used.value) if used.value else b""
        finally:
            self.L.ntc_buffer_free(out)
        out = (list(metas)[:nb], payload, int(nbases.value))
        if non_acgt is not None:
            out += (self.exceptions(),)
        if qualities is not None:
            out += (self.qualities(),)
        if names is not None:
            out += (self.names(),)
        if digests is not None:
            out += (self.encode_digests(),)
        return out

    # ---- paired-end reads ---------------------------------------------------------------
    @property
    def paired(self):
        """Option "paired" (PAIR_MODES): 0 off, 1 reads 2p and 2p + 1 are mates and their ids are
        checked at encode, 2 mates without the check.  Set, encode_pack_fastq takes interleaved
        text and decode_fasta_unpacked returns the two parts."""
        return self.get_option("paired")

    @paired.setter
    def paired(self, mode):
        self.set_option("paired", _pair_code(mode))

    def encode_pack_fastq_paired(self, text1, text2, n_pairs, block_reads=65536, non_acgt=None, qualities=None,
                                 names=None, quality_coder=None, digests=None, quality_smooth=None,
                                 quality_smooth_to=None):
        """encode_pack_fastq of the two mate texts woven on the GPU
        (ntc_encode_pack_fastq_paired): record p of text1, then record p of text2.  Needs
        `paired` set; returns what encode_pack_fastq returns for the interleaved text."""
        t1 = np.frombuffer(bytes(text1), dtype=np.uint8) if len(text1) else np.zeros(1, dtype=np.uint8)
        t2 = np.frombuffer(bytes(text2), dtype=np.uint8) if len(text2) else np.zeros(1, dtype=np.uint8)
        nb = (2 * n_pairs + block_reads - 1) // block_reads
        metas = (BlockMeta * max(nb, 1))()
        out, used, nbases, bad = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int64(-1)
        with self._policy(non_acgt), self._qmode(qualities), self._nmode(names), self._qcoder(quality_coder), \
                self._digests(digests), self._qsmooth(quality_smooth), self._qsmooth_to(quality_smooth_to):
            rc = self.L.ntc_encode_pack_fastq_paired(self.h, _p(t1), len(text1), _p(t2), len(text2), n_pairs,
                                                     block_reads, metas, ctypes.byref(out), ctypes.byref(used),
                                                     ctypes.byref(nbases), ctypes.byref(bad))
        if rc:
            self.L.ntc_buffer_free(out)
            e = NtcError(rc, self.L.ntc_last_error(self.h).decode(errors="replace"))
            e.bad_read = bad.value
            raise e
        try:
            payload = ctypes.string_at(out.value, used.value) if used.value else b""
        finally:
            self.L.ntc_buffer_free(out)
        out = (list(metas)[:nb], payload, int(nbases.value))
        if non_acgt is not None:
            out += (self.exceptions(),)
        if qualities is not None:
            out += (self.qualities(),)
        if names is not None:
            out += (self.names(),)
        if digests is not None:
            out += (self.encode_digests(),)
        return out

    def pair_split(self):
        """Bytes of part 1 of the last paired text decode (ntc_decode_pair_split)."""
        first = ctypes.c_uint64()
        self._check(self.L.ntc_decode_pair_split(self.h, ctypes.byref(first)), "ntc_decode_pair_split")
        return int(first.value)

    def set_window(self, first, count):
        """Only reads [first, first + count) of the next decode_fasta / decode_fasta_unpacked
        batch are formatted (ntc_decode_set_window); the batch is still decoded and checked
        whole, and the reads keep their ids, names and qualities."""
        self._check(self.L.ntc_decode_set_window(self.h, int(first), int(count)), "ntc_decode_set_window")

    def encode_status(self):
        bad, n = ctypes.c_int64(-1), ctypes.c_uint64()
        self._check(self.L.ntc_encode_status(self.h, ctypes.byref(bad), ctypes.byref(n)), "ntc_encode_status")
        return int(n.value)

    def decode_device(self, d_recs, n_recs, d_out, out_cap, d_offs, offs_cap):
        self._check(self.L.ntc_decode_batch_device(self.h, ctypes.c_void_p(d_recs), n_recs, ctypes.c_void_p(d_out),
                                                   out_cap, ctypes.c_void_p(d_offs), offs_cap),
                    "ntc_decode_batch_device")

    def decode_status(self):
        nr, nb = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.L.ntc_decode_status(self.h, ctypes.byref(nr), ctypes.byref(nb)), "ntc_decode_status")
        return int(nr.value), int(nb.value)

    def unpack(self, metas, payload, n_blocks=None):
        """GPU unpacker (ntc_unpack_streams): blocks' inflated streams -> records in HBM ->
        (blocks decoded before the first damaged one, reads, bases)."""
        n = len(metas) if n_blocks is None else n_blocks
        buf = np.frombuffer(bytes(payload), dtype=np.uint8) if len(payload) else np.zeros(8, dtype=np.uint8)
        ok, nr, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.L.ntc_unpack_streams(self.h, _p(buf), len(payload), ctypes.cast(metas, ctypes.c_void_p), n,
                                              ctypes.byref(ok), ctypes.byref(nr), ctypes.byref(nb)),
                    "ntc_unpack_streams")
        return int(ok.value), int(nr.value), int(nb.value)

    def unpacked_records(self):
        n = ctypes.c_uint64()
        self.L.ntc_unpacked_records(self.h, None, 0, ctypes.byref(n))
        out = np.zeros(max(1, n.value), dtype=np.uint64)
        self._check(self.L.ntc_unpacked_records(self.h, _p(out), len(out), ctypes.byref(n)), "ntc_unpacked_records")
        return out[:n.value]

    def decode_fasta_unpacked(self, first_id=1, bgzf=None):
        """The text of the records the last unpack left (ntc_decode_fasta_unpacked); paired: its two
        parts.  bgzf (None: as the context's bgzf_text stands): True for BGZF members in place of the
        text, for this call; bgzf_last() then has their table."""
        if bgzf is not None and bool(bgzf) != self.bgzf_text:
            was = self.bgzf_text
            self.bgzf_text = bgzf
            try:
                return self.decode_fasta_unpacked(first_id)
            finally:
                self.bgzf_text = was
        need = ctypes.c_uint64()
        rc = self.L.ntc_decode_fasta_unpacked(self.h, first_id, None, 0, ctypes.byref(need))
        if rc not in (0, 5):
            self._check(rc, "ntc_decode_fasta_unpacked")
        out = np.zeros(max(1, need.value), dtype=np.uint8)
        self._check(self.L.ntc_decode_fasta_unpacked(self.h, first_id, _p(out), len(out), ctypes.byref(need)),
                    "ntc_decode_fasta_unpacked")
        text = out[:need.value].tobytes()
        if self.paired and not self.get_option("discard_text"):  # the two parts: all mate-1 records, all mate-2 records
            first = self.pair_split()
            return text[:first], text[first:]
        return text

    def synchronize(self):
        self._check(self.L.ntc_ctx_synchronize(self.h), "ntc_ctx_synchronize")

    def timing(self):
        t = Timing()
        self._check(self.L.ntc_last_timing(self.h, ctypes.byref(t)), "ntc_last_timing")
        return {"total_ms": t.total_ms, "main_ms": t.main_ms, "aux_ms": t.aux_ms}


# ---- reference-shaped helpers --------------------------------------------------------
def encode_sequence(nucleotides, ctx):
    """encode_sequence + encode_dictionary for one read -> list of u64 records."""
    bases, offs = pack_reads([nucleotides])
    recs, _ = ctx.encode(bases, offs)
    return [int(x) for x in recs]


def decode_sequence(encoding, ctx):
    """decode_sequence: u64 records of whole reads -> list of bytes (one per read)."""
    out, offs = ctx.decode(np.asarray(encoding, dtype=np.uint64))
    return [out[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]


def synth_genome(seed, length):
    out = np.zeros(length, dtype=np.uint8)
    rc = lib().ntc_synth_genome(seed, length, _p(out))
    if rc:
        raise NtcError(rc, "ntc_synth_genome")
    return out


def synth_strains(genome, seed, n_strains, snp_per_million):
    """n_strains mutated copies of genome (i.i.d. substitutions), as one (n_strains, len) array."""
    genome = np.ascontiguousarray(genome, dtype=np.uint8)
    out = np.zeros((n_strains, len(genome)), dtype=np.uint8)
    rc = lib().ntc_synth_strains(_p(genome), len(genome), seed, n_strains, snp_per_million, _p(out))
    if rc:
        raise NtcError(rc, "ntc_synth_strains")
    return out


def minimizer_keys(reads, n_reads, read_len, w=20, threads=0):
    """smallest hashed w-mer of each read (bench.py --presort locality experiment)"""
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    keys = np.zeros(n_reads, dtype=np.uint64)
    rc = lib().ntc_minimizer_keys(_p(reads), n_reads, read_len, w, threads, _p(keys))
    if rc:
        raise NtcError(rc, "ntc_minimizer_keys")
    return keys


def synth_reads(genome, seed, first_read, n_reads, read_len, err_per_million, threads=0):
    genome = np.ascontiguousarray(genome, dtype=np.uint8)
    out = np.zeros(n_reads * read_len, dtype=np.uint8)
    rc = lib().ntc_synth_reads(_p(genome), len(genome), seed, first_read, n_reads, read_len, err_per_million,
                               threads, _p(out))
    if rc:
        raise NtcError(rc, "ntc_synth_reads")
    return out


# ---- block container (encoded.dat) ------------------------------------------------------
def file_header():
    """encode_file_header(0,0,0,0): 32 zero bytes (lib.rs:52-67)."""
    buf = (ctypes.c_uint8 * 32)()
    lib().ntc_file_header(buf)
    return bytes(buf)


def write_block(records, num_records):
    """write_block_to (lib.rs:232-252) -> bytes of the 4 (header, gzip payload) blocks.
    Raises NtcError(NTC_ERR_EMPTY_READ) where the reference's write_block_to errs (and
    its CLI then silently drops the block)."""
    recs = np.ascontiguousarray(records, dtype=np.uint64)
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    rc = lib().ntc_write_block(_p(recs), len(recs), num_records, ctypes.byref(out), ctypes.byref(n))
    if rc:
        raise NtcError(rc, "ntc_write_block")
    try:
        return ctypes.string_at(out.value, n.value)
    finally:
        lib().ntc_buffer_free(out)


def pack_block(records, num_records):
    """The part of write_block_to before deflate (split_encoded_dictionary + Rice /
    minimal-binary coding, encode.rs:59-94,168-229) on the host -> (BlockMeta, payload
    bytes).  meta.status = NTC_ERR_EMPTY_READ (3) for a block the reference drops."""
    recs = np.ascontiguousarray(records, dtype=np.uint64)
    meta, out, n = BlockMeta(), ctypes.c_void_p(), ctypes.c_uint64()
    rc = lib().ntc_pack_block(_p(recs) if len(recs) else None, len(recs), num_records, ctypes.byref(meta),
                              ctypes.byref(out), ctypes.byref(n))
    if rc not in (0, 3):
        raise NtcError(rc, "ntc_pack_block")
    try:
        return meta, (ctypes.string_at(out.value, n.value) if out.value else b"")
    finally:
        lib().ntc_buffer_free(out)


class IndexPrep:
    """The host half of an upload (ntc_index_prepare): the index's derived tables, built
    without a GPU -- e.g. while contexts are created -- and uploaded to each context with
    GpuContext.upload_prepared."""

    def __init__(self, index):
        self.h = ctypes.c_void_p()
        self._index = index  # the view's arrays stay alive
        rc = lib().ntc_index_prepare(ctypes.byref(index.view), ctypes.byref(self.h))
        if rc:
            raise NtcError(rc, "ntc_index_prepare")

    def close(self):
        if self.h:
            lib().ntc_index_prep_free(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stream_payloads(meta, payload):
    """The four streams' pre-deflate bytes of a packed block."""
    return [bytes(payload[m.offset:m.offset + 8 * m.encoded_size]) for m in meta.stream]


def deflate_block(meta, payload, engine="zlib"):
    """Headers + gzip members of a packed block (the bytes write_block_to writes)."""
    buf = np.frombuffer(payload, dtype=np.uint8) if len(payload) else np.zeros(1, dtype=np.uint8)
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    rc = lib().ntc_deflate_block(ctypes.byref(meta), _p(buf), DEFLATE_ENGINES[engine], ctypes.byref(out),
                                 ctypes.byref(n))
    if rc:
        raise NtcError(rc, "ntc_deflate_block")
    try:
        return ctypes.string_at(out.value, n.value)
    finally:
        lib().ntc_buffer_free(out)


def deflate_stream(meta, stream, payload, engine="zlib"):
    """One stream's header + gzip member (ntc_deflate_stream); the four concatenated are
    deflate_block's bytes."""
    buf = np.frombuffer(payload, dtype=np.uint8) if len(payload) else np.zeros(1, dtype=np.uint8)
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    rc = lib().ntc_deflate_stream(ctypes.byref(meta), stream, _p(buf), DEFLATE_ENGINES[engine], ctypes.byref(out),
                                  ctypes.byref(n))
    if rc:
        raise NtcError(rc, "ntc_deflate_stream")
    try:
        return ctypes.string_at(out.value, n.value)
    finally:
        lib().ntc_buffer_free(out)


# ---- inflate of gzip members of at most 64 KiB (ntc_inflate_members, include/ntcomp_codec.h) ----
INFLATE_MAX_OUT = 65536
INFLATE_MEMBER = np.dtype([("src_off", "<u8"), ("src_bytes", "<u4"), ("out_bytes", "<u4"), ("dst_off", "<u8")])
INFLATE_RESULT = np.dtype([("status", "<u4"), ("out_bytes", "<u4"), ("crc", "<u4"), ("reserved", "<u4")])
INFLATE_STATUS = {0: "ok", 1: "bad header", 2: "bad block", 3: "bad code", 4: "bad distance", 5: "output overrun",
                  6: "input overrun", 7: "CRC mismatch", 8: "ISIZE mismatch", 9: "too large"}


def bgzf_members(blob):
    """The BGZF members at the start of blob -> list of (offset, size, ISIZE).  A member is a gzip
    member with FEXTRA whose extra field holds the subfield 'B' 'C' of two bytes, BSIZE = size - 1;
    the list ends at the first bytes that are no such member, or whose size passes the blob."""
    blob = memoryview(blob)
    out, at, n = [], 0, len(blob)
    while n - at >= 18 and bytes(blob[at:at + 4]) == b"\x1f\x8b\x08\x04":
        xlen = blob[at + 10] | blob[at + 11] << 8
        p, end, size = at + 12, at + 12 + xlen, None
        while p + 4 <= min(end, n):
            slen = blob[p + 2] | blob[p + 3] << 8
            if blob[p] == 66 and blob[p + 1] == 67 and slen == 2 and p + 6 <= min(end, n):
                size = (blob[p + 4] | blob[p + 5] << 8) + 1
                break
            p += 4 + slen
        if size is None or size < xlen + 12 + 8 or at + size > n:
            break
        out.append((at, size, int.from_bytes(blob[at + size - 4:at + size], "little")))
        at += size
    return out


# ---- BGZF members of a text (ntc_bgzf_compress, include/ntcomp_codec.h) ----
BGZF_MEMBER_BYTES = 65280  # text bytes per member at most
BGZF_GRID = 61440          # grid step of the record-aligned cuts
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BGZF_MEMBER = np.dtype([("text_off", "<u8"), ("text_bytes", "<u8"), ("place", "<u8"), ("bytes", "<u8")])


def bgzf_members_max(n):
    """The most members the plan makes of n bytes, whatever the record offsets."""
    return -(-n // BGZF_GRID) + n // BGZF_MEMBER_BYTES


def bgzf_bound(n):
    """ntc_bgzf_bound: the most bytes the members of an n-byte text take."""
    return int(lib().ntc_bgzf_bound(n))


def bgzf_compress(text, rec_off=None, ctx=None, cap=None):
    """The BGZF members of text (ntc_bgzf_compress): on ctx's GPU, or with ctx None through the
    host restatement, same bytes.  rec_off (None: plain 65,280-byte cuts): the records' offsets,
    first 0 and last len(text); the members then end on record boundaries.  No EOF member is
    appended (BGZF_EOF).  Returns (the members' bytes, a BGZF_MEMBER array).  cap: the output
    capacity to offer (default: the bound); NtcError(NTC_ERR_CAPACITY) carries .needed."""
    n = len(text)
    src = np.frombuffer(bytes(text), dtype=np.uint8) if n else np.zeros(1, dtype=np.uint8)
    off = None if rec_off is None else np.ascontiguousarray(rec_off, dtype=np.uint64)
    if off is not None and len(off) == 0:
        raise ValueError("rec_off holds at least one offset")
    cap = bgzf_bound(n) if cap is None else cap
    out = np.zeros(max(1, cap), dtype=np.uint8)
    tab = np.zeros(max(1, bgzf_members_max(n)), dtype=BGZF_MEMBER)
    nm, used = ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib().ntc_bgzf_compress(ctx.h if ctx is not None else None, _p(src), n, None if off is None else _p(off),
                                 0 if off is None else len(off) - 1, _p(out), cap, _p(tab), len(tab), ctypes.byref(nm),
                                 ctypes.byref(used))
    if rc:
        e = NtcError(rc, lib().ntc_last_error(ctx.h).decode(errors="replace") if ctx is not None else "ntc_bgzf_compress")
        e.needed = int(used.value)
        raise e
    return out[:used.value].tobytes(), tab[:nm.value].copy()


def _inflate_descs(members):
    if isinstance(members, np.ndarray) and members.dtype == INFLATE_MEMBER:
        return np.ascontiguousarray(members)
    m = np.zeros(len(members), dtype=INFLATE_MEMBER)
    at = 0
    for i, t in enumerate(members):
        if len(t) == 3:  # (offset, size, ISIZE) as bgzf_members lists them: the outputs back to back
            m[i] = (t[0], t[1], t[2], at)
            at += t[2]
        else:
            m[i] = tuple(t)
    return m


def inflate_members(ctx, blob, members, out=None):
    """Inflate gzip members of blob (ntc_inflate_members): on ctx's GPU, or with ctx None through the
    decoder's host restatement.  members: an INFLATE_MEMBER array, tuples (src_off, src_bytes,
    out_bytes, dst_off), or bgzf_members' triples (their outputs then lie back to back).  Returns
    (the output as a uint8 array, an INFLATE_RESULT array); a member whose status is not 0 leaves
    its bytes of the output as they were (zeros, or what `out` held)."""
    m = _inflate_descs(members)
    src = np.frombuffer(bytes(blob), dtype=np.uint8) if len(blob) else np.zeros(1, dtype=np.uint8)
    if out is None:
        out = np.zeros(int(max((int(d["dst_off"]) + int(d["out_bytes"]) for d in m), default=0)), dtype=np.uint8)
    res = np.zeros(len(m), dtype=INFLATE_RESULT)
    bad = ctypes.c_uint64()
    rc = lib().ntc_inflate_members(ctx.h if ctx is not None else None, _p(src), len(blob), _p(m) if len(m) else None, len(m),
                                   _p(out) if len(out) else None, len(out), _p(res) if len(m) else None, ctypes.byref(bad))
    if rc:
        raise NtcError(rc, lib().ntc_last_error(ctx.h).decode(errors="replace") if ctx is not None else "ntc_inflate_members")
    assert int(bad.value) == int((res["status"] != 0).sum())
    return out, res


def read_block(data):
    """One block of decode_block (lib.rs:320-363) -> (u64 records, bytes consumed,
    num_records header field).  NtcError(NTC_ERR_IO) at a clean end of input."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    used, recs, n, nrec = ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib().ntc_read_block(_p(buf), len(data), ctypes.byref(used), ctypes.byref(recs), ctypes.byref(n),
                              ctypes.byref(nrec))
    if rc:
        raise NtcError(rc, "ntc_read_block")
    try:
        arr = np.ctypeslib.as_array((ctypes.c_uint64 * n.value).from_address(recs.value)).copy() \
            if n.value else np.zeros(0, dtype=np.uint64)
    finally:
        lib().ntc_buffer_free(recs)
    return arr, int(used.value), int(nrec.value)


def read_block_streams(data):
    """The host half of decode_block for the GPU unpacker (ntc_read_block_streams): one
    block's stream headers + inflated streams -> (BlockMeta, payload bytes, bytes consumed).
    NtcError(NTC_ERR_IO) at a clean end of input."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    used, meta = ctypes.c_uint64(), BlockMeta()
    # the payload is at most 8x the gzip'd bytes' inflated size; ask the headers first
    cap = 0
    pos = 0
    for _ in range(4):
        if pos + 32 > len(data):
            break
        h = bytes(data[pos:pos + 32])
        cap += 8 * int.from_bytes(h[12:16], "little")
        pos += 32 + int.from_bytes(h[0:4], "little")
    pay = np.zeros(max(cap, 8), dtype=np.uint8)
    rc = lib().ntc_read_block_streams(_p(buf), len(data), ctypes.byref(used), _p(pay), cap, ctypes.byref(meta))
    if rc:
        raise NtcError(rc, "ntc_read_block_streams")
    return meta, pay[:cap].tobytes(), int(used.value)


def concat_streams(blocks):
    """(meta, payload) pairs -> one payload and the metas with their offsets moved into it
    (each block's streams stay 8-byte aligned): the input of GpuContext.unpack."""
    metas = (BlockMeta * max(1, len(blocks)))()
    parts, off = [], 0
    for i, (m, pay) in enumerate(blocks):
        mm = BlockMeta()
        ctypes.memmove(ctypes.byref(mm), ctypes.byref(m), ctypes.sizeof(BlockMeta))
        for s in range(4):
            mm.stream[s].offset = m.stream[s].offset + off
        metas[i] = mm
        pad = (-len(pay)) % 8
        parts.append(bytes(pay) + b"\0" * pad)
        off += len(pay) + pad
    return metas, b"".join(parts)


# ---- FASTX ingest ---------------------------------------------------------------------
def encode_file(ctxs, in_path, out_fd, threads=0, blocks_per_batch=4, batch_bases=0, deflate="zlib",
                host_parse=False, non_acgt=None, nx_fd=-1, qualities=None, q_fd=-1, names=None, n_fd=-1, d_fd=None,
                mate_path=None, pair_mode=None, inflate="host"):
    """`ntcomp encode` file to file (ntc_encode_file, include/ntcomp_pipeline.h): FASTX ->
    GPU encode + block packer on every context -> deflate pool -> encoded.dat on out_fd.
    A plain FASTQ is parsed on the GPU unless host_parse.  Returns the per-stage stats as
    a dict (gpu_parsed = batches parsed on the GPU); raises NtcError (with .bad_read).
    non_acgt ("error", "mask", "keep"; ntc_encode_file_nx): what becomes of N and IUPAC
    symbols; "keep" writes their exception runs to nx_fd, and the stats gain an "nx" dict
    (ntc_nx_stats).  qualities ("drop", "keep", "bin8"; ntc_encode_file_ex): "keep" and "bin8"
    write the blocks' quality sections to q_fd ("NTCQ"), and the stats gain a "q" dict
    (ntc_q_stats).  names ("drop", "keep", "id"; ntc_encode_file_ex2): "keep" and "id" write the
    blocks' name sections to n_fd ("NTCN"), and the stats gain an "n" dict (ntc_n_stats).  d_fd (None:
    no digests; ntc_encode_file_ex3): the blocks' content digests, computed on the GPU, go to that
    descriptor ("NTCD"), and the stats gain a "d" dict (ntc_d_stats).  pair_mode ("ids", "nocheck";
    ntc_encode_file_ex4): the reads are pairs, in_path interleaved, or with mate_path the mate-1 file
    beside the mate-2 file mate_path (then pair_mode defaults to "ids"); the stats gain a "p" dict
    (ntc_p_stats).  inflate ("host", "gpu"; ntc_encode_file_ex6): under "gpu" the runs of members of a
    BGZF input are inflated on the first context's device, the output is byte for byte that of
    "host", and the stats gain an "i" dict (ntc_i_stats)."""
    o = PipelineOpts(threads, blocks_per_batch, batch_bases, DEFLATE_ENGINES[deflate], 1 if host_parse else 0)
    if mate_path is not None and pair_mode is None:
        pair_mode = "ids"
    pairs = _pair_code(pair_mode) if pair_mode is not None else 0
    if INFLATE_ENGINES[inflate]:
        fo = FileOpts6(ctypes.sizeof(FileOpts6), _policy_code(non_acgt or 0), nx_fd, _quality_code(qualities or 0), q_fd, None,
                       None, _names_code(names or 0), n_fd, None, 0 if d_fd is None else 1, -1 if d_fd is None else d_fd, None,
                       pairs, None if mate_path is None else os.fsencode(mate_path), -1, 0, 0, INFLATE_ENGINES[inflate], 0)
        side = [("nx", NxStats()), ("q", QStats()), ("n", NStats()), ("d", DStats()), ("p", PStats()), ("i", IStats())]
        d = _run_pipeline("ntc_encode_file_ex6", ctxs, in_path, out_fd, o, mid=(ctypes.byref(fo),),
                          tail=tuple(ctypes.byref(s) for _, s in side))
        asked = {"nx": True, "q": qualities is not None, "n": names is not None, "d": d_fd is not None, "p": bool(pairs), "i": True}
        d.update({key: _stats_dict(s) for key, s in side if asked[key]})
        return d
    level = 4 if pairs else 3 if d_fd is not None else 2 if names is not None else 1 if qualities is not None else 0
    if level == 0 and non_acgt is None:
        return _run_pipeline("ntc_encode_file", ctxs, in_path, out_fd, o)
    side = [("nx", NxStats()), ("q", QStats()), ("n", NStats()), ("d", DStats()), ("p", PStats())][:level + 1]
    if level == 0:
        fn, mid = "ntc_encode_file_nx", (_policy_code(non_acgt), nx_fd)
    else:
        fo = _file_opts(level, (_policy_code(non_acgt or 0), nx_fd, _quality_code(qualities or 0), q_fd, None, None,
                                _names_code(names or 0), n_fd, None, 0 if d_fd is None else 1, -1 if d_fd is None else d_fd,
                                None, pairs, None if mate_path is None else os.fsencode(mate_path), -1))
        fn, mid = _LEVELS[level].format("encode"), (ctypes.byref(fo),)
    d = _run_pipeline(fn, ctxs, in_path, out_fd, o, mid=mid, tail=tuple(ctypes.byref(s) for _, s in side))
    asked = {"nx": True, "q": qualities is not None, "n": names is not None, "d": d_fd is not None, "p": True}
    d.update({key: _stats_dict(s) for key, s in side if asked[key]})
    return d


def decode_file(ctxs, in_path, out_fd, threads=0, blocks_per_batch=2, nx_path=None, q_path=None, n_path=None,
                d_path=None, out_fd2=-1, pair_mode=None, reads=None, out_format="text"):
    """`ntcomp decode` file to file (ntc_decode_file, include/ntcomp_pipeline.h): encoded.dat
    -> inflate + stream decode pool -> GPU inverse-SBWT walk + FASTA formatting on every
    context -> FASTA on out_fd.  Stats as a dict; a damaged block ends the output after the
    blocks before it without an error, like decode_block's Err ends the reference's loop
    (src/main.rs:202): stats["dropped_blocks"] > 0 and stats["error"] say so.  nx_path: the
    exception side file written by encode_file(non_acgt="keep"), whose symbols are put back
    (ntc_decode_file_nx).  q_path: the quality side file written by encode_file(qualities=
    "keep" / "bin8"); the output is then FASTQ (ntc_decode_file_ex).  n_path: the name side file
    written by encode_file(names="keep" / "id"); the reads then carry their names instead of
    seq.N (ntc_decode_file_ex2).  d_path: the digest file written by encode_file(d_fd=...): every
    block is checked on the GPU against it (ntc_decode_file_ex3); NtcError(NTC_ERR_DIGEST) with
    .bad_read = the first read of the block that differs, or for a file written against another
    index; a damaged or truncated input is then NTC_ERR_FORMAT; the stats gain a "d" dict
    (ntc_d_stats).  With d_path, out_fd -1 checks without copying or writing the text.  pair_mode
    ("ids" or "nocheck": the archive holds pairs; ntc_decode_file_ex4): the mate-1 records go to
    out_fd and the mate-2 records to out_fd2; the stats gain a "p" dict (ntc_p_stats).
    reads=(first, count): only that range of the archive's reads, counted from 0
    (ntc_decode_file_ex5; count 0 = the whole file): the blocks that hold it are decoded, the
    reads keep their numbers, names and qualities, and the stats gain an "r" dict (ntc_r_stats).
    A range is strict: a damaged block at or before it, or a side file that does not describe the
    archive's blocks, is NTC_ERR_FORMAT; a range the archive does not hold is
    NTC_ERR_INVALID_ARG.  out_format "bgzf" (ntc_decode_file_ex7): every batch's text is cut into
    BGZF members at record boundaries and compressed on the GPU; out_fd (and out_fd2) get the
    members and, when the call succeeds, the EOF member; the stats gain a "z" dict (ntc_z_stats)."""
    o = PipelineOpts(threads, blocks_per_batch, 0, 0, 0)
    pairs = _pair_code(pair_mode) if pair_mode is not None else 0
    if OUT_FORMATS[out_format]:
        enc = lambda p: None if p is None else os.fsencode(p)
        first, count = (int(x) for x in reads) if reads is not None else (0, 0)
        fo = FileOpts7(ctypes.sizeof(FileOpts7), 0, -1, 0, -1, enc(nx_path), enc(q_path), 0, -1, enc(n_path), 0, -1, enc(d_path),
                       pairs, None, out_fd2, first, count, 0, 0, OUT_FORMATS[out_format], 0)
        side = [("d", DStats()), ("p", PStats()), ("r", RStats()), ("z", ZStats())]
        try:
            d = _run_pipeline("ntc_decode_file_ex7", ctxs, in_path, out_fd, o, mid=(ctypes.byref(fo),),
                              tail=tuple(ctypes.byref(s) for _, s in side))
        except NtcError as e:
            e.stats["d"] = side[0][1].as_dict()
            raise
        asked = {"d": d_path is not None, "p": bool(pairs), "r": reads is not None, "z": True}
        d.update({key: _stats_dict(s) for key, s in side if asked[key]})
        return d
    level = 5 if reads is not None else 4 if pairs else 3 if d_path is not None else 2 if n_path is not None else 1 if q_path is not None else 0
    if level == 0:
        if nx_path is None:
            return _run_pipeline("ntc_decode_file", ctxs, in_path, out_fd, o)
        return _run_pipeline("ntc_decode_file_nx", ctxs, in_path, out_fd, o, pre_fd=(os.fsencode(nx_path),))
    enc = lambda p: None if p is None else os.fsencode(p)
    fo = _file_opts(level, (0, -1, 0, -1, enc(nx_path), enc(q_path), 0, -1, enc(n_path), 0, -1, enc(d_path), pairs, None,
                            out_fd2) + (tuple(int(x) for x in reads) if reads is not None else ()))
    side = [("d", DStats()), ("p", PStats()), ("r", RStats())][:max(0, level - 2)]
    try:
        d = _run_pipeline(_LEVELS[level].format("decode"), ctxs, in_path, out_fd, o, mid=(ctypes.byref(fo),),
                          tail=tuple(ctypes.byref(s) for _, s in side))
    except NtcError as e:
        if side:
            e.stats["d"] = side[0][1].as_dict()
        raise
    asked = {"d": d_path is not None, "p": bool(pairs), "r": True}
    d.update({key: _stats_dict(s) for key, s in side if asked[key]})
    return d


def archive_info(path):
    """The blocks of an encoded.dat from their headers alone (ntc_archive_info; host only, no
    context): {"blocks": [{"offset", "bytes", "reads", "records", "bad"}, ...], "n_blocks",
    "n_reads", "n_records", "tail_bytes"}.  A bad block (damaged headers) counts no reads."""
    p, nb, nr, nrec, tail = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib().ntc_archive_info(os.fsencode(path), ctypes.byref(p), ctypes.byref(nb), ctypes.byref(nr),
                                ctypes.byref(nrec), ctypes.byref(tail))
    if rc:
        raise NtcError(rc, f"ntc_archive_info: {path}")
    try:
        arr = ctypes.cast(p, ctypes.POINTER(ArchiveBlock))
        blocks = [arr[i].as_dict() for i in range(nb.value)]
    finally:
        lib().ntc_buffer_free(p)
    return {"blocks": blocks, "n_blocks": int(nb.value), "n_reads": int(nr.value), "n_records": int(nrec.value),
            "tail_bytes": int(tail.value)}


def shard_blocks(i, n, n_blocks):
    """Blocks [lo, hi) of the i-th (from 1) of n contiguous slices of n_blocks whole blocks:
    [(i - 1) n_blocks / n, i n_blocks / n), rounded down.  The n slices partition the blocks."""
    if not 1 <= i <= n:
        raise ValueError(f"shard {i}/{n}: need 1 <= I <= N")
    return (i - 1) * n_blocks // n, i * n_blocks // n


def read_exceptions(path):
    """An exception side file ("NTCX", include/ntcomp_codec.h) parsed and validated by
    ntc_nx_read -> (runs of dtype NX_RUN, substitute base as an int); NtcError(NTC_ERR_FORMAT)
    if it is malformed."""
    p, n, sub = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint32()
    rc = lib().ntc_nx_read(os.fsencode(path), ctypes.byref(p), ctypes.byref(n), ctypes.byref(sub))
    if rc:
        raise NtcError(rc, f"ntc_nx_read({path})")
    try:
        runs = (np.frombuffer(ctypes.string_at(p.value, n.value * NX_RUN.itemsize), dtype=NX_RUN).copy()
                if n.value else np.zeros(0, dtype=NX_RUN))
    finally:
        lib().ntc_buffer_free(p)
    return runs, int(sub.value)


def read_qualities(path):
    """The quality side file ("NTCQ", include/ntcomp_codec.h) written beside an encoded.dat:
    ntc_q_read -> (mode as an int, list of QualMeta, the inflated words as bytes);
    NtcError(NTC_ERR_FORMAT) for a malformed file."""
    mode, pm, nb, pp, nbytes = ctypes.c_int(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_uint64()
    rc = lib().ntc_q_read(os.fsencode(path), ctypes.byref(mode), ctypes.byref(pm), ctypes.byref(nb), ctypes.byref(pp),
                          ctypes.byref(nbytes))
    if rc:
        raise NtcError(rc, f"ntc_q_read({path})")
    try:
        metas = [QualMeta.from_buffer_copy(ctypes.string_at(pm.value + i * ctypes.sizeof(QualMeta), ctypes.sizeof(QualMeta)))
                 for i in range(nb.value)]
        payload = ctypes.string_at(pp.value, nbytes.value) if nbytes.value else b""
    finally:
        lib().ntc_buffer_free(pm)
        lib().ntc_buffer_free(pp)
    return int(mode.value), metas, payload


def write_qualities(fd, mode, metas, payload, header=True, engine="libdeflate", coder="pack"):
    """The "NTCQ" header (when header) and one section per QualMeta to fd (ntc_q_write_header2,
    ntc_q_write_section); payload: the words the metas' payload_off point into.  coder "rans":
    the version-2 header, for sections whose metas say coder 1."""
    if header:
        rc = lib().ntc_q_write_header2(fd, _quality_code(mode), _coder_code(coder))
        if rc:
            raise NtcError(rc, "ntc_q_write_header2")
    buf = np.frombuffer(bytes(payload), dtype=np.uint8) if len(payload) else np.zeros(8, dtype=np.uint8)
    for m in metas:
        if m.payload_off + m.payload_bytes > len(payload):
            raise NtcError(1, "section outside the payload")
        rc = lib().ntc_q_write_section(fd, ctypes.byref(m), ctypes.c_void_p(buf.ctypes.data + m.payload_off),
                                       DEFLATE_ENGINES[engine])
        if rc:
            raise NtcError(rc, "ntc_q_write_section")


def read_names(path):
    """The name side file ("NTCN", include/ntcomp_codec.h) written beside an encoded.dat:
    ntc_n_read -> (mode as an int, list of NameMeta, the inflated payload as bytes);
    NtcError(NTC_ERR_FORMAT) for a malformed file."""
    mode, pm, nb, pp, nbytes = ctypes.c_int(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_uint64()
    rc = lib().ntc_n_read(os.fsencode(path), ctypes.byref(mode), ctypes.byref(pm), ctypes.byref(nb), ctypes.byref(pp),
                          ctypes.byref(nbytes))
    if rc:
        raise NtcError(rc, f"ntc_n_read({path})")
    try:
        metas = [NameMeta.from_buffer_copy(ctypes.string_at(pm.value + i * ctypes.sizeof(NameMeta), ctypes.sizeof(NameMeta)))
                 for i in range(nb.value)]
        payload = ctypes.string_at(pp.value, nbytes.value) if nbytes.value else b""
    finally:
        lib().ntc_buffer_free(pm)
        lib().ntc_buffer_free(pp)
    return int(mode.value), metas, payload


def write_names(fd, mode, metas, payload, header=True, engine="libdeflate"):
    """The "NTCN" header (when header) and one section per NameMeta to fd (ntc_n_write_header,
    ntc_n_write_section); payload: the bytes the metas' payload_off point into."""
    if header:
        rc = lib().ntc_n_write_header(fd, _names_code(mode))
        if rc:
            raise NtcError(rc, "ntc_n_write_header")
    buf = np.frombuffer(bytes(payload), dtype=np.uint8) if len(payload) else np.zeros(8, dtype=np.uint8)
    for m in metas:
        if m.payload_off + m.payload_bytes > len(payload):
            raise NtcError(1, "section outside the payload")
        rc = lib().ntc_n_write_section(fd, ctypes.byref(m), ctypes.c_void_p(buf.ctypes.data + m.payload_off),
                                       DEFLATE_ENGINES[engine])
        if rc:
            raise NtcError(rc, "ntc_n_write_section")


def read_digests(path):
    """The digest side file ("NTCD", include/ntcomp_codec.h) written beside an encoded.dat:
    ntc_d_read -> (components, k, n_nodes, list of DigestMeta); NtcError(NTC_ERR_FORMAT) for a
    malformed file."""
    comp, k, n, pm, nb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_uint64()
    rc = lib().ntc_d_read(os.fsencode(path), ctypes.byref(comp), ctypes.byref(k), ctypes.byref(n), ctypes.byref(pm),
                          ctypes.byref(nb))
    if rc:
        raise NtcError(rc, f"ntc_d_read({path})")
    try:
        size = ctypes.sizeof(DigestMeta)
        metas = [DigestMeta.from_buffer_copy(ctypes.string_at(pm.value + i * size, size)) for i in range(nb.value)]
    finally:
        lib().ntc_buffer_free(pm)
    return int(comp.value), int(k.value), int(n.value), metas


def write_digests(fd, components, k, n_nodes, metas, header=True):
    """The "NTCD" header (when header) and one section per DigestMeta to fd (ntc_d_write_header,
    ntc_d_write_section)."""
    if header:
        rc = lib().ntc_d_write_header(fd, components, k, n_nodes)
        if rc:
            raise NtcError(rc, "ntc_d_write_header")
    for m in metas:
        rc = lib().ntc_d_write_section(fd, ctypes.byref(m))
        if rc:
            raise NtcError(rc, "ntc_d_write_section")


def write_exceptions(fd, runs, sub, header=True):
    """The side file's header (if header) and one section holding runs (if any) to fd
    (ntc_nx_write); sections may follow one another, in (read, pos) order over the file."""
    runs = np.ascontiguousarray(runs, dtype=NX_RUN)
    sub = sub if isinstance(sub, int) else ord(sub)
    rc = lib().ntc_nx_write(fd, _p(runs) if len(runs) else None, len(runs), sub, 1 if header else 0)
    if rc:
        raise NtcError(rc, "ntc_nx_write")


# the entry points that take an ntc_file_opts struct, by level, and their struct
_LEVELS = {1: "ntc_{}_file_ex", 2: "ntc_{}_file_ex2", 3: "ntc_{}_file_ex3", 4: "ntc_{}_file_ex4",
           5: "ntc_{}_file_ex5"}  # (decode only)


def _file_opts(level, values):
    """The ntc_file_opts struct of a level from the values of ntc_file_opts5's fields (after
    struct_bytes) in order: each level's struct holds a prefix of them."""
    cls = (FileOpts, FileOpts2, FileOpts3, FileOpts4, FileOpts5)[level - 1]
    if level == 1:
        return cls(*values[:len(cls._fields_)])
    return cls(ctypes.sizeof(cls), *values[:len(cls._fields_) - 1])


def _stats_dict(s):
    return s.as_dict() if hasattr(s, "as_dict") else {k: int(getattr(s, k)) for k, _ in s._fields_}


def _run_pipeline(fn, ctxs, in_path, out_fd, o, pre_fd=(), mid=(), tail=()):
    arr = (ctypes.c_void_p * len(ctxs))(*[c.h.value for c in ctxs])
    st = PipelineStats()
    rc = getattr(lib(), fn)(arr, len(ctxs), os.fsencode(in_path), *pre_fd, out_fd, *mid, ctypes.byref(o),
                            ctypes.byref(st), *tail)
    d = {k: (getattr(st, k).decode(errors="replace") if k == "error" else getattr(st, k))
         for k, _ in PipelineStats._fields_}
    if rc:
        e = NtcError(rc, d["error"])
        e.bad_read = d["bad_read"]
        e.stats = d
        raise e
    return d


def libdeflate_available():
    """libdeflate.so.0 loads on this host (the block codec's fast deflate engine)."""
    try:
        ctypes.CDLL("libdeflate.so.0")
        return True
    except OSError:
        return False


def host_threads():
    """CPUs this process may use (NTC_THREADS, else min(affinity, cgroup CPU quota))."""
    return int(lib().ntc_host_threads())


class FastxReader:
    """needletail::parse_fastx_file + normalize(true) (src/main.rs:51-62, 158-163): plain or
    gzip FASTA/FASTQ -> batches of (bases, read offsets) as numpy arrays (copies)."""

    def __init__(self, path):
        self.h = ctypes.c_void_p()
        rc = lib().ntc_fastx_open(os.fsencode(path), ctypes.byref(self.h))
        if rc:
            raise NtcError(rc, f"ntc_fastx_open({path})")

    def batch(self, max_reads=1 << 20, max_bases=1 << 28):
        b, o, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
        rc = lib().ntc_fastx_next_batch(self.h, max_reads, max_bases, ctypes.byref(b), ctypes.byref(o), ctypes.byref(n))
        if rc:
            raise NtcError(rc, "ntc_fastx_next_batch")
        if n.value == 0:
            return None
        offs = np.ctypeslib.as_array((ctypes.c_uint64 * (n.value + 1)).from_address(o.value)).copy()
        total = int(offs[-1])
        bases = (np.ctypeslib.as_array((ctypes.c_uint8 * total).from_address(b.value)).copy() if total
                 else np.zeros(0, dtype=np.uint8))
        return bases, offs

    def __iter__(self):
        while True:
            x = self.batch()
            if x is None:
                return
            yield x

    def close(self):
        if self.h:
            lib().ntc_fastx_close(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fasta_format(bases, offsets, first_id):
    """Decode output lines (src/main.rs:203-209): '>seq.{first_id + r}' + read r."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    b = bases if len(bases) else np.zeros(1, dtype=np.uint8)
    rc = lib().ntc_fasta_format(_p(b), _p(offsets), len(offsets) - 1, first_id, ctypes.byref(out), ctypes.byref(n))
    if rc:
        raise NtcError(rc, "ntc_fasta_format")
    try:
        return ctypes.string_at(out.value, n.value)
    finally:
        lib().ntc_buffer_free(out)
