"""ctypes binding of libamphora_hip.so (the C ABI in include/amphora.h).

This is the product path: every arithmetic call goes to the HIP kernels.
There is no CPU fallback -- if the shared library is missing or cannot be
loaded, importing this module raises.

Buffers: host calls take C-contiguous numpy uint8 arrays (or bytes); device
calls take torch uint8 tensors on the context's GPU and run asynchronously on
torch's current stream (so torch.cuda.Event timing sees them).
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libamphora_hip.so")

AMPH_OK, AMPH_E_VERIFY, AMPH_E_LEN, AMPH_E_PARAM, AMPH_E_HIP, AMPH_E_NOMEM, AMPH_E_RANGE = 0, 1, 2, 3, 4, 5, 6
AMPH_F_DEVICE = 1
AMPH_F_ACCUMULATE = 2
AMPH_NO_FAILURE = 0x7F7F7F7F7F7F7F7F
MAX_PARTIES = 16


class AmphoraNativeError(RuntimeError):
    def __init__(self, status: int, detail: str):
        super().__init__("%s (status %d): %s" % (_STATUS.get(status, "error"), status, detail))
        self.status = status


def _need(cond: bool, detail: str):
    """Host-side length check of a call whose C entry point takes raw pointers
    and one word count (it cannot see the buffers' sizes)."""
    if not cond:
        raise AmphoraNativeError(AMPH_E_LEN, detail)


_STATUS = {AMPH_E_VERIFY: "verification failed", AMPH_E_LEN: "length invariant",
           AMPH_E_PARAM: "invalid argument", AMPH_E_HIP: "HIP error", AMPH_E_NOMEM: "out of memory",
           AMPH_E_RANGE: "array index out of range"}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("libamphora_hip.so not built (%s): run `python tools/build_native.py` "
                          "or __graft_entry__.build(); there is no CPU fallback" % LIB_PATH)
    # torch (if present) ships its own libamdhip64.so.7; loading it first makes
    # this library bind to the same HIP runtime instance (same SONAME), so
    # device pointers and streams from torch are valid here.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    vp, sz, i32, u32, u64, i64p = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_int64)
    L.amph_ctx_create.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, i32, C.POINTER(vp)]
    L.amph_ctx_create_multi.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(i32), i32,
                                        C.POINTER(vp)]
    L.amph_ctx_device_count.argtypes = [vp]
    L.amph_ctx_destroy.argtypes = [vp]
    L.amph_ctx_device.argtypes = [vp]
    L.amph_ctx_set_batch_words.argtypes = [vp, sz]
    L.amph_ctx_stats.argtypes = [vp, vp]
    L.amph_strerror.restype = C.c_char_p
    L.amph_strerror.argtypes = [i32]
    L.amph_last_error.restype = C.c_char_p
    L.amph_version.restype = C.c_char_p
    L.amph_build_id.restype = C.c_char_p
    L.amph_recombine_verify.argtypes = [vp, vp, i32, vp, i64p, u32, vp]
    L.amph_mask_input.argtypes = [vp, vp, i32, vp, sz, vp, i64p, u32, vp]
    L.amph_recombine_verify_packed.argtypes = [vp, vp, i32, vp, sz, vp, vp, u32, vp]
    L.amph_mask_input_packed.argtypes = [vp, vp, i32, vp, sz, vp, vp, vp, u32, vp]
    L.amph_recombine_verify_batch.argtypes = [vp, vp, i32, sz, C.POINTER(vp), i64p, u32]
    L.amph_mask_input_batch.argtypes = [vp, vp, i32, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), i64p, u32]
    L.amph_recombine.argtypes = [vp, C.POINTER(vp), i32, sz, vp, u32, vp]
    L.amph_recombine_object.argtypes = [vp, C.POINTER(vp), i32, C.POINTER(sz), vp, u32, vp]
    L.amph_verify.argtypes = [vp, vp, vp, vp, vp, vp, sz, i64p, u32, vp]
    L.amph_verify_message.argtypes = [vp, vp, vp, vp, vp, vp, C.c_char_p, sz]
    L.amph_mask_words.argtypes = [vp, vp, vp, sz, vp, u32, vp]
    L.amph_mask_word_host.argtypes = [vp, C.c_char_p, C.c_char_p, vp]
    L.amph_to_gfp.argtypes = [vp, vp, sz, vp, u32, vp]
    L.amph_from_gfp.argtypes = [vp, vp, sz, vp, u32, vp]
    L.amph_convert_share.argtypes = [vp, vp, vp, sz, C.c_char_p, i32, vp, u32, vp]
    L.amph_odo_pre.argtypes = [vp, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, u32, vp]
    L.amph_open_diffs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i32, sz, vp, u32, vp]
    L.amph_odo_post.argtypes = [vp, vp, vp, sz, i32, vp, vp, u32, vp]
    L.amph_open_post.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i32, vp, sz, i32, vp, vp, u32, vp]
    L.amph_host_register.argtypes = [vp, vp, sz]
    L.amph_host_unregister.argtypes = [vp, vp]
    L.amph_time_next_launch.argtypes = [vp, vp]
    L.amph_timing_event_create.argtypes = [C.POINTER(vp)]
    L.amph_timing_event_destroy.argtypes = [vp]
    L.amph_timing_event_record.argtypes = [vp, vp]
    L.amph_timing_event_elapsed_ms.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.amph_base64_encode.argtypes = [vp, vp, sz, vp, u32, vp]
    L.amph_base64_decode.argtypes = [vp, vp, sz, vp, C.POINTER(C.c_size_t), i64p, u32, vp]
    L.amph_base64_encode_words.argtypes = [vp, vp, sz, vp, u32, vp]
    L.amph_base64_decode_words.argtypes = [vp, vp, sz, vp, i64p, u32, vp]
    L.amph_exchange_max_chars.restype = sz
    L.amph_exchange_max_chars.argtypes = [sz]
    L.amph_exchange_encode.argtypes = [vp, vp, vp, sz, vp, sz, vp, u32, vp]
    L.amph_exchange_decode.argtypes = [vp, vp, sz, sz, vp, vp, i64p, u32, vp]
    L.amph_synth_odos.argtypes = [vp, u64, i32, sz, C.POINTER(vp), vp, C.c_int64, i32, vp]
    L.amph_synth_words.argtypes = [vp, u64, sz, vp, vp]
    L.amph_stream_probe.argtypes = [vp, vp, i32, vp, sz, vp, vp]
    L.amph_recombine_verify_b64.argtypes = [vp, vp, i32, sz, vp, i64p, i64p, u32, vp]
    L.amph_mask_input_b64.argtypes = [vp, vp, i32, sz, vp, sz, vp, vp, i64p, i64p, u32, vp]
    L.amph_masked_input_data_chars.restype = sz
    L.amph_masked_input_data_chars.argtypes = [sz]
    L.amph_convert_share_json.argtypes = [vp, vp, sz, sz, vp, C.c_char_p, i32, vp, i64p, u32, vp]
    L.amph_mask_input_json.argtypes = [vp, vp, i32, sz, vp, sz, vp, sz, i64p, i64p, u32, vp]
    L.amph_party_begin.argtypes = [vp, vp, sz, vp, vp, sz, i32, vp, vp, vp, C.POINTER(vp)]
    L.amph_party_words.restype = sz
    L.amph_party_words.argtypes = [vp]
    L.amph_party_text_len.restype = u64
    L.amph_party_text_len.argtypes = [vp]
    L.amph_party_text.argtypes = [vp, vp, sz]
    L.amph_party_partner.argtypes = [vp, i32, vp, sz, i64p]
    L.amph_party_finish.argtypes = [vp, i32, vp, vp]
    L.amph_party_finish_b64.argtypes = [vp, i32, C.POINTER(vp)]
    L.amph_party_free.restype = None
    L.amph_party_free.argtypes = [vp]
    L.amph_party_begin_dev.argtypes = [vp, vp, sz, vp, vp, sz, i32, vp, vp, vp, vp, C.POINTER(vp)]
    L.amph_party_text_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.amph_party_partner_dev.argtypes = [vp, i32, vp, sz, vp, vp]
    L.amph_party_finish_b64_dev.argtypes = [vp, i32, C.POINTER(vp), vp]
    L.amph_party_reset_partner.argtypes = [vp, i32]
    # include/amphora_wire_batch.h
    pp = C.POINTER(vp)
    L.amph_wire_slot_chars.restype = sz
    L.amph_wire_slot_chars.argtypes = [sz]
    L.amph_wire_batch_copies.restype = u64
    L.amph_wire_batch_copies.argtypes = [vp]
    L.amph_recombine_verify_b64_packed.argtypes = [vp, vp, i32, vp, vp, sz, vp, vp, vp, u32, vp]
    L.amph_mask_input_b64_packed.argtypes = [vp, vp, i32, vp, vp, sz, vp, vp, vp, vp, vp, u32, vp]
    L.amph_recombine_verify_b64_batch.argtypes = [vp, vp, i32, sz, C.POINTER(sz), pp, i64p, i64p, u32]
    L.amph_mask_input_b64_batch.argtypes = [vp, vp, i32, sz, C.POINTER(sz), pp, pp, pp, i64p, i64p, u32]
    # include/amphora_upload_batch.h
    L.amph_upload_slot_chars.restype = sz
    L.amph_upload_slot_chars.argtypes = [sz]
    L.amph_upload_batch_copies.restype = u64
    L.amph_upload_batch_copies.argtypes = [vp]
    L.amph_convert_share_json_packed.argtypes = [vp, vp, sz, vp, vp, sz, vp, C.c_char_p, i32, vp, vp, u32, vp]
    L.amph_convert_share_json_batch.argtypes = [vp, pp, C.POINTER(sz), C.POINTER(sz), sz, pp, C.c_char_p, i32, pp,
                                                i64p, u32]
    L.amph_mask_input_json_packed.argtypes = [vp, vp, i32, vp, vp, sz, vp, vp, sz, vp, vp, vp, u32, vp]
    L.amph_mask_input_json_batch.argtypes = [vp, vp, i32, sz, C.POINTER(sz), pp, pp, i64p, i64p, u32]
    # include/amphora_respond_batch.h
    L.amph_respond_batch_copies.restype = u64
    L.amph_respond_batch_copies.argtypes = [vp]
    L.amph_odo_fields_b64_packed.argtypes = [vp, vp, vp, vp, sz, vp, vp, u32, vp]
    L.amph_odo_fields_b64_batch.argtypes = [vp, vp, sz, pp, vp, u32]
    # include/amphora_exchange_batch.h
    L.amph_exchange_slot_chars.restype = sz
    L.amph_exchange_slot_chars.argtypes = [sz]
    L.amph_exchange_batch_copies.restype = u64
    L.amph_exchange_batch_copies.argtypes = [vp]
    L.amph_exchange_encode_packed.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp, sz, vp, u32, vp]
    L.amph_exchange_decode_packed.argtypes = [vp, vp, sz, vp, vp, vp, sz, sz, vp, vp, vp, u32, vp]
    L.amph_exchange_encode_batch.argtypes = [vp, pp, pp, C.POINTER(sz), sz, pp, C.POINTER(sz), vp, u32]
    L.amph_exchange_decode_batch.argtypes = [vp, pp, C.POINTER(sz), C.POINTER(sz), sz, pp, pp, i64p, u32]
    # include/amphora_party_batch.h
    L.amph_parties_begin.argtypes = [vp, vp, sz, vp, vp, vp, sz, i32, vp, vp, vp, pp]
    L.amph_parties_begin_dev.argtypes = [vp, vp, sz, vp, vp, vp, sz, i32, vp, vp, vp, vp, pp]
    for f in (L.amph_parties_objects, L.amph_parties_words, L.amph_parties_text_bytes, L.amph_parties_field_chars):
        f.restype = sz
        f.argtypes = [vp]
    L.amph_parties_text_offsets.argtypes = [vp, vp]
    L.amph_parties_field_offsets.argtypes = [vp, vp]
    L.amph_parties_text_lens.argtypes = [vp, vp]
    L.amph_parties_text.argtypes = [vp, sz, vp, sz]
    L.amph_parties_text_dev.argtypes = [vp, pp, pp, pp]
    L.amph_parties_partner.argtypes = [vp, i32, vp, vp, vp]
    L.amph_parties_partner_dev.argtypes = [vp, i32, vp, vp, vp, vp]
    L.amph_parties_reset_partner.argtypes = [vp, i32]
    L.amph_parties_finish.argtypes = [vp, i32, vp, vp]
    L.amph_parties_finish_b64.argtypes = [vp, i32, pp, vp]
    L.amph_parties_finish_b64_dev.argtypes = [vp, i32, pp, vp]
    L.amph_parties_free.restype = None
    L.amph_parties_free.argtypes = [vp]
    # include/amphora_client_session.h
    L.amph_client_begin.argtypes = [vp, sz, i32, pp]
    L.amph_client_begin_dev.argtypes = [vp, sz, i32, vp, pp]
    L.amph_client_party.argtypes = [vp, i32, vp, i64p]
    L.amph_client_party_dev.argtypes = [vp, i32, vp, i64p, vp]
    L.amph_client_finish_verify.argtypes = [vp, vp, i64p, i64p]
    L.amph_client_finish_verify_dev.argtypes = [vp, vp, i64p, i64p, vp]
    L.amph_client_finish_mask.argtypes = [vp, vp, sz, vp, vp, i64p, i64p]
    L.amph_client_finish_mask_dev.argtypes = [vp, vp, sz, vp, vp, i64p, i64p, vp]
    L.amph_client_finish_mask_json.argtypes = [vp, vp, sz, vp, sz, i64p, i64p]
    L.amph_client_finish_mask_json_dev.argtypes = [vp, vp, sz, vp, sz, i64p, i64p, vp]
    L.amph_client_word.argtypes = [vp, sz, vp]
    L.amph_client_words.restype = sz
    L.amph_client_words.argtypes = [vp]
    L.amph_client_parties_seen.argtypes = [vp]
    L.amph_client_free.restype = None
    L.amph_client_free.argtypes = [vp]
    # include/amphora_client_batch.h
    L.amph_clients_begin.argtypes = [vp, vp, sz, i32, pp]
    L.amph_clients_begin_dev.argtypes = [vp, vp, sz, i32, vp, pp]
    for f in (L.amph_clients_objects, L.amph_clients_words, L.amph_clients_field_chars,
              L.amph_clients_upload_chars):
        f.restype = sz
        f.argtypes = [vp]
    L.amph_clients_parties_seen.argtypes = [vp]
    L.amph_clients_field_offsets.argtypes = [vp, vp]
    L.amph_clients_upload_offsets.argtypes = [vp, vp]
    L.amph_clients_party.argtypes = [vp, i32, vp, vp]
    L.amph_clients_party_dev.argtypes = [vp, i32, vp, vp, vp]
    L.amph_clients_finish_verify.argtypes = [vp, vp, vp, vp]
    L.amph_clients_finish_verify_dev.argtypes = [vp, vp, vp, vp, vp]
    L.amph_clients_finish_mask.argtypes = [vp, vp, vp, vp, vp, vp]
    L.amph_clients_finish_mask_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.amph_clients_finish_mask_json.argtypes = [vp, vp, vp, sz, vp, vp]
    L.amph_clients_finish_mask_json_dev.argtypes = [vp, vp, vp, sz, vp, vp, vp]
    L.amph_clients_word.argtypes = [vp, sz, sz, vp]
    L.amph_clients_copies.restype = u64
    L.amph_clients_copies.argtypes = [vp]
    L.amph_clients_free.restype = None
    L.amph_clients_free.argtypes = [vp]
    # include/amphora_client_bodies.h
    L.amph_bodies_scan.argtypes = [C.c_char_p, sz, vp, vp]
    L.amph_bodies_party.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(sz), vp]
    L.amph_bodies_party_dev.argtypes = [vp, i32, vp, sz, vp, vp]
    return L


lib = _load()


def build_id() -> str:
    """The id compiled into the loaded library (amph_build_id)."""
    return lib.amph_build_id().decode()


def tree_build_id() -> str:
    """The id of the source tree beside the library (tools/build_native.py
    tree_digest over the same sources, headers, flags and arch)."""
    root = os.path.dirname(HERE)
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import build_native
    finally:
        sys.path.pop(0)
    return build_native.tree_digest()


def check_build_id() -> str:
    """Raise unless the loaded library was built from this tree; returns the id."""
    got, want = build_id(), tree_build_id()
    if got != want:
        raise RuntimeError("libamphora_hip.so carries build id %s but the sources beside it hash to %s: "
                           "rebuild (__graft_entry__.build())" % (got, want))
    return got

EXPORTED = ["amph_ctx_create", "amph_ctx_create_multi", "amph_ctx_device_count",
            "amph_ctx_destroy", "amph_ctx_device", "amph_ctx_set_batch_words", "amph_ctx_stats", "amph_strerror",
            "amph_last_error", "amph_version", "amph_build_id", "amph_recombine_verify", "amph_mask_input",
            "amph_recombine_verify_packed", "amph_mask_input_packed", "amph_recombine_verify_batch",
            "amph_mask_input_batch",
            "amph_recombine", "amph_recombine_object", "amph_verify", "amph_verify_message", "amph_mask_words", "amph_mask_word_host",
            "amph_to_gfp", "amph_from_gfp", "amph_convert_share", "amph_odo_pre",
            "amph_open_diffs", "amph_odo_post", "amph_open_post", "amph_synth_odos", "amph_synth_words",
            "amph_host_register", "amph_host_unregister", "amph_time_next_launch",
            "amph_timing_event_create", "amph_timing_event_destroy", "amph_timing_event_record",
            "amph_timing_event_elapsed_ms", "amph_base64_encode", "amph_base64_decode",
            "amph_base64_encode_words", "amph_base64_decode_words", "amph_exchange_max_chars",
            "amph_exchange_encode", "amph_exchange_decode", "amph_stream_probe",
            "amph_recombine_verify_b64", "amph_mask_input_b64", "amph_masked_input_data_chars",
            "amph_convert_share_json", "amph_mask_input_json", "amph_party_begin", "amph_party_words", "amph_party_text_len",
            "amph_party_text", "amph_party_partner", "amph_party_finish", "amph_party_finish_b64",
            "amph_party_free", "amph_party_begin_dev", "amph_party_text_dev", "amph_party_partner_dev",
            "amph_party_finish_b64_dev", "amph_party_reset_partner"]
# what include/amphora_wire_batch.h declares (the extension header keeps its own list)
EXPORTED_WIRE_BATCH = ["amph_wire_slot_chars", "amph_wire_batch_copies", "amph_recombine_verify_b64_packed",
                       "amph_mask_input_b64_packed", "amph_recombine_verify_b64_batch",
                       "amph_mask_input_b64_batch"]
# what include/amphora_upload_batch.h declares
EXPORTED_UPLOAD_BATCH = ["amph_upload_slot_chars", "amph_upload_batch_copies", "amph_convert_share_json_packed",
                         "amph_convert_share_json_batch", "amph_mask_input_json_packed",
                         "amph_mask_input_json_batch"]
# what include/amphora_respond_batch.h declares
EXPORTED_RESPOND_BATCH = ["amph_odo_fields_b64_packed", "amph_odo_fields_b64_batch", "amph_respond_batch_copies"]
# what include/amphora_exchange_batch.h declares
EXPORTED_EXCHANGE_BATCH = ["amph_exchange_slot_chars", "amph_exchange_encode_packed", "amph_exchange_encode_batch",
                           "amph_exchange_decode_packed", "amph_exchange_decode_batch",
                           "amph_exchange_batch_copies"]
AMPH_EXCHANGE_SLOT_ALIGN = 8192
# what include/amphora_party_batch.h declares
EXPORTED_PARTY_BATCH = ["amph_parties_begin", "amph_parties_begin_dev", "amph_parties_objects", "amph_parties_words",
                        "amph_parties_text_bytes", "amph_parties_field_chars", "amph_parties_text_offsets",
                        "amph_parties_field_offsets", "amph_parties_text_lens", "amph_parties_text",
                        "amph_parties_text_dev", "amph_parties_partner", "amph_parties_partner_dev",
                        "amph_parties_reset_partner", "amph_parties_finish", "amph_parties_finish_b64",
                        "amph_parties_finish_b64_dev", "amph_parties_free"]
AMPH_PARTIES_ALL = (1 << (8 * C.sizeof(C.c_size_t))) - 1
# what include/amphora_client_session.h declares
EXPORTED_CLIENT_SESSION = ["amph_client_begin", "amph_client_party", "amph_client_finish_verify",
                           "amph_client_finish_mask", "amph_client_finish_mask_json", "amph_client_word",
                           "amph_client_words", "amph_client_parties_seen", "amph_client_free",
                           "amph_client_begin_dev", "amph_client_party_dev", "amph_client_finish_verify_dev",
                           "amph_client_finish_mask_dev", "amph_client_finish_mask_json_dev"]
# what include/amphora_client_batch.h declares
EXPORTED_CLIENTS_SESSION = ["amph_clients_begin", "amph_clients_begin_dev", "amph_clients_objects",
                            "amph_clients_words", "amph_clients_parties_seen", "amph_clients_field_chars",
                            "amph_clients_upload_chars", "amph_clients_field_offsets",
                            "amph_clients_upload_offsets", "amph_clients_party", "amph_clients_party_dev",
                            "amph_clients_finish_verify", "amph_clients_finish_verify_dev",
                            "amph_clients_finish_mask", "amph_clients_finish_mask_dev",
                            "amph_clients_finish_mask_json", "amph_clients_finish_mask_json_dev",
                            "amph_clients_word", "amph_clients_copies", "amph_clients_free"]
# what include/amphora_client_bodies.h declares
EXPORTED_CLIENT_BODIES = ["amph_bodies_scan", "amph_bodies_party", "amph_bodies_party_dev"]
AMPH_BODY_ABSENT = (1 << 64) - 1
ODO_FIELD_NAMES = ("secretShares", "rShares", "vShares", "wShares", "uShares")


class BodyNotPlain(ValueError):
    """amph_bodies_scan refused a body (anything but the plain form): the
    caller parses it its own way (wire.odo_field_texts)."""


def bodies_scan(body: bytes):
    """amph_bodies_scan: -> (starts[5], lens[5]) (uint64 arrays) of the five
    top-level base64 members of one response body, in ODO order; raises
    BodyNotPlain with the scanner's reason for anything but the plain form."""
    out = np.empty((2, 5), np.uint64)
    st = lib.amph_bodies_scan(body, len(body), out[0].ctypes.data, out[1].ctypes.data)
    if st == AMPH_E_PARAM:
        raise BodyNotPlain(lib.amph_last_error().decode())
    Context._check(st)
    return out[0], out[1]


def wire_text_chars(words: int) -> int:
    """Characters of the base64 text of `words` 16-byte words, padding included."""
    return 4 * ((16 * words + 2) // 3)


def wire_slot_chars(words: int) -> int:
    """amph_wire_slot_chars: the text rounded up to whole 16-character units."""
    return int(lib.amph_wire_slot_chars(words))


def masked_input_data_chars(words: int) -> int:
    """Characters of the MaskedInput "data" array text of `words` compact records."""
    return 37 * words + 1 if words else 2


def upload_slot_chars(words: int) -> int:
    """amph_upload_slot_chars: that text rounded up to whole 16-byte units."""
    return int(lib.amph_upload_slot_chars(words))


def exchange_slot_chars(npairs: int) -> int:
    """amph_exchange_slot_chars: amph_exchange_max_chars rounded up to AMPH_EXCHANGE_SLOT_ALIGN."""
    return int(lib.amph_exchange_slot_chars(npairs))


def wire_bad_char_message(bad: int, words: int) -> str:
    """The single wire-text call's message for a bad_char verdict of an object
    of `words` words ((5 party + field) * nchars + offset)."""
    nc = wire_text_chars(words)
    return "Illegal base64 character at index %d of party %d's %s" % (
        bad % nc, bad // nc // 5, ODO_FIELD_NAMES[bad // nc % 5])


class TimingEvent:
    """A timing-only hipEvent_t (amph_timing_event_create: no system-scope
    fence on record) for amph_time_next_launch."""

    def __init__(self):
        h = C.c_void_p()
        Context._check(lib.amph_timing_event_create(C.byref(h)))
        self.handle = h

    def elapsed_ms(self, stop: "TimingEvent") -> float:
        ms = C.c_float()
        Context._check(lib.amph_timing_event_elapsed_ms(self.handle, stop.handle, C.byref(ms)))
        return ms.value

    def __del__(self):
        if getattr(self, "handle", None) is not None and lib is not None:
            lib.amph_timing_event_destroy(self.handle)
            self.handle = None


class _AmphOdo(C.Structure):
    _fields_ = [("secret_shares", C.c_void_p), ("r_shares", C.c_void_p), ("v_shares", C.c_void_p),
                ("w_shares", C.c_void_p), ("u_shares", C.c_void_p), ("nbytes", C.c_size_t)]


class _AmphStats(C.Structure):  # amph_stats
    _fields_ = [(k, C.c_uint64) for k in ("kernel_launches", "pool_buffers", "pool_bytes",
                                           "device_workers", "worker_tasks")]


class _AmphOdoB64Out(C.Structure):  # amph_odo_b64_out: five writable field buffers of nchars capacity each
    _fields_ = [("secret_shares", C.c_void_p), ("r_shares", C.c_void_p), ("v_shares", C.c_void_p),
                ("w_shares", C.c_void_p), ("u_shares", C.c_void_p), ("nchars", C.c_size_t)]


class _AmphOdoB64(C.Structure):  # amph_odo_b64: one party's five base64 field texts
    _fields_ = [("secret_shares", C.c_void_p), ("r_shares", C.c_void_p), ("v_shares", C.c_void_p),
                ("w_shares", C.c_void_p), ("u_shares", C.c_void_p), ("nchars", C.c_size_t)]


def le16(x: int) -> bytes:
    return int(x).to_bytes(16, "little")


def _is_dev(x) -> bool:
    return hasattr(x, "is_cuda") and x.is_cuda


def words_view(x, width: int = 16):
    """bytes / bytearray / numpy -> C-contiguous uint8 numpy array (n, width)."""
    if _is_dev(x):
        return x
    if isinstance(x, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(x), np.uint8)
    else:
        a = np.ascontiguousarray(x, dtype=np.uint8)
    n = a.size // width
    return a.reshape(-1)[: n * width].reshape(n, width)


def byte_len(x) -> int:
    """Length in bytes of a word buffer as the caller passed it (a ragged
    party's array need not hold whole words)."""
    if _is_dev(x):
        return x.numel() * x.element_size()
    if isinstance(x, (bytes, bytearray, memoryview)):
        return memoryview(x).nbytes
    # the same conversion words_view makes: the length of the uint8 buffer whose
    # pointer goes to C (an int64 array is 8x its converted size in nbytes)
    return int(np.ascontiguousarray(x, dtype=np.uint8).size)


def _ptr(x):
    if x is None:
        return None
    if _is_dev(x):
        return x.data_ptr()
    return x.ctypes.data


class Context:
    """One amph_ctx: field parameters (prime, r, rInv) bound to one GPU."""

    def __init__(self, prime: int, r: int, r_inv: int, device: int = 0, devices=None):
        """devices: several GPU ordinals -> amph_ctx_create_multi (host-pointer
        calls are sharded over them); device-pointer calls use devices[0]."""
        if devices is not None and len(devices) > 0:
            device = int(devices[0])
        self.prime, self.r, self.r_inv, self.device = prime, r, r_inv, device
        h = C.c_void_p()
        keys = (le16(prime % (1 << 128)), le16(r % (1 << 128)), le16(r_inv % (1 << 128)))
        if devices is not None and len(devices) > 1:
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            self._check(lib.amph_ctx_create_multi(*keys, arr, len(devices), C.byref(h)))
        else:
            self._check(lib.amph_ctx_create(*keys, device, C.byref(h)))
        self._h = h

    @property
    def device_count(self) -> int:
        return lib.amph_ctx_device_count(self._h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.amph_ctx_destroy(h)
            self._h = None

    @staticmethod
    def _check(st: int, allow_verify: bool = False):
        if st == AMPH_OK or (allow_verify and st == AMPH_E_VERIFY):
            return st
        raise AmphoraNativeError(st, lib.amph_last_error().decode())

    def stats(self) -> dict:
        """amph_ctx_stats: kernel launches, pooled party buffers, device workers."""
        st = _AmphStats()
        self._check(lib.amph_ctx_stats(self._h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in _AmphStats._fields_}

    def set_batch_words(self, words: int):
        self._check(lib.amph_ctx_set_batch_words(self._h, words))

    def host_register(self, array: np.ndarray):
        """Page-lock a numpy buffer so host-pointer calls DMA it directly."""
        self._check(lib.amph_host_register(self._h, array.ctypes.data, array.nbytes))

    def host_unregister(self, array: np.ndarray):
        self._check(lib.amph_host_unregister(self._h, array.ctypes.data))

    # -- mode plumbing ----------------------------------------------------------
    def _mode(self, *arrays):
        dev = [_is_dev(a) for a in arrays if a is not None]
        if any(dev) and not all(dev):
            raise ValueError("mix of host and device buffers")
        if dev and dev[0]:
            import torch
            return AMPH_F_DEVICE, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return 0, None

    def _empty(self, like, shape, dtype="uint8"):
        if _is_dev(like):
            import torch
            return torch.empty(shape, dtype=getattr(torch, dtype), device=like.device)
        return np.empty(shape, dtype=dtype)

    def _ff(self, like):
        if _is_dev(like):
            import torch
            t = torch.empty(1, dtype=torch.int64, device=like.device)
            return t, C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_int64))
        v = C.c_int64(-1)
        return v, C.pointer(v)

    @staticmethod
    def _ff_value(ff):
        if isinstance(ff, C.c_int64):
            return ff.value
        return ff  # device tensor: AMPH_NO_FAILURE or index, read by the caller

    def _bad_char_status(self, st, sv, n_secrets, words, bad) -> bool:
        """AMPH_E_PARAM of amph_mask_input_b64 / _json that reports a bad base64
        character (the wrapper raises ValueError for it).  Host mode: bad_char
        is set.  Device mode reports one only with n_secrets > words, after it
        has waited for the verdicts, and names it in amph_last_error."""
        if st != AMPH_E_PARAM:
            return False
        if not _is_dev(sv):
            return self._ff_value(bad) >= 0
        return n_secrets > words and lib.amph_last_error().startswith(b"Illegal base64 character")

    def _odo_structs(self, odos):
        n = len(odos)
        arr = (_AmphOdo * n)()
        views = []
        for j, o in enumerate(odos):
            lens = [byte_len(f) for f in o]
            if len(lens) != 5 or any(b != lens[0] for b in lens):
                # OutputDeliveryObject's constructor invariant (OutputDeliveryObject.java:90-96)
                raise AmphoraNativeError(AMPH_E_LEN, "The provided shares must be of the same length")
            fs = [words_view(f) for f in o]
            views.append(fs)
            # the party's own byte length: parties may differ (recombineObject's
            # ragged semantics, include/amphora.h amph_odo)
            arr[j] = _AmphOdo(*[_ptr(f) for f in fs], lens[0])
        return arr, views

    def _out(self, like, shape, out):
        """A fresh output buffer, or the caller's `out` (same memory kind,
        C-contiguous uint8 of exactly `shape`) so repeated calls reuse one
        (page-locked, if the caller registered it) buffer."""
        if out is None:
            return self._empty(like, shape)
        if _is_dev(out) != _is_dev(like):
            raise ValueError("out must live where the inputs live")
        ok = (tuple(out.shape) == tuple(shape) and str(out.dtype).endswith("uint8") and
              (out.is_contiguous() if _is_dev(out) else out.flags["C_CONTIGUOUS"]))
        if not ok:
            raise ValueError("out must be a C-contiguous uint8 array of shape %r" % (shape,))
        return out

    # -- client --------------------------------------------------------------
    def recombine_verify(self, odos, out=None):
        """odos: list over parties of (y, r, v, w, u) word arrays.
        Returns (canonical secrets (W,16), first_fail) -- first_fail is -1 /
        index on the host path, an int64[1] device tensor on the device path."""
        arr, views = self._odo_structs(odos)
        flags, stream = self._mode(*[f for v in views for f in v])
        W = arr[0].nbytes // 16  # party 0's word count (SecretShareUtil.java:75)
        out = self._out(views[0][0], (W, 16), out)
        ff, ffp = self._ff(views[0][0])
        self._check(lib.amph_recombine_verify(self._h, arr, len(odos), _ptr(out), ffp, flags,
                                              stream), allow_verify=True)
        return out, self._ff_value(ff)

    def mask_input(self, mask_odos, secrets16, out=None):
        arr, views = self._odo_structs(mask_odos)
        s = words_view(secrets16)
        flags, stream = self._mode(s, *[f for v in views for f in v])
        out = self._out(s, (s.shape[0], 16), out)
        ff, ffp = self._ff(s)
        self._check(lib.amph_mask_input(self._h, arr, len(mask_odos), _ptr(s), s.shape[0],
                                        _ptr(out), ffp, flags, stream), allow_verify=True)
        return out, self._ff_value(ff)

    # -- many secrets in one call (include/amphora.h, "many secrets in one call") --
    def _packed(self, masked, odos, offsets, secrets16, out, first_fail, accumulate):
        arr, views = self._odo_structs(odos)
        s = words_view(secrets16) if masked else None
        like = views[0][0]
        flags, stream = self._mode(s, *[f for v in views for f in v])
        T = arr[0].nbytes // 16
        out = self._out(like, (T, 16), out)
        if flags & AMPH_F_DEVICE:
            import torch
            if not _is_dev(offsets):
                offsets = torch.as_tensor(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to(like.device)
            if offsets.element_size() != 8 or not offsets.is_contiguous():
                raise ValueError("offsets must be a contiguous 8-byte integer tensor")
            K = max(0, offsets.numel() - 1)
            if first_fail is None:
                first_fail = torch.empty(K, dtype=torch.int64, device=like.device)
                accumulate = False
            elif first_fail.numel() != K or first_fail.dtype != torch.int64 or not first_fail.is_cuda:
                raise ValueError("first_fail must be an int64 device tensor with one entry per object")
            if accumulate:
                flags |= AMPH_F_ACCUMULATE
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            K = max(0, offsets.size - 1)
            first_fail = np.full(K, -1, dtype=np.int64)
        if masked:
            _need(s.shape[0] == T, "the packed form takes one secret per input mask word")
            st = lib.amph_mask_input_packed(self._h, arr, len(odos), _ptr(offsets), K, _ptr(s), _ptr(out),
                                            _ptr(first_fail), flags, stream)
        else:
            st = lib.amph_recombine_verify_packed(self._h, arr, len(odos), _ptr(offsets), K, _ptr(out),
                                                  _ptr(first_fail), flags, stream)
        self._check(st, allow_verify=True)
        return out, first_fail

    def recombine_verify_packed(self, odos, offsets, out=None, first_fail=None, accumulate=False):
        """K secrets in one launch.  odos: list over parties of (y, r, v, w, u),
        each the concatenation of the K objects' words; offsets: K + 1 word
        offsets (numpy, or a device tensor beside device fields).  Returns
        (secrets (T, 16), first_fail): host -- int64[K] of -1 / the object's
        smallest failing local word; device -- an int64[K] tensor of
        AMPH_NO_FAILURE / index (pass first_fail with accumulate=True to
        min-combine into an earlier call's verdicts)."""
        return self._packed(False, odos, offsets, None, out, first_fail, accumulate)

    def mask_input_packed(self, mask_odos, offsets, secrets16, out=None, first_fail=None, accumulate=False):
        """recombine_verify_packed over Input Mask ODOs fused with maskInput:
        one secret per mask word, packed on the same offsets."""
        return self._packed(True, mask_odos, offsets, secrets16, out, first_fail, accumulate)

    def _batch(self, masked, objects, secrets):
        K = len(objects)
        n = len(objects[0]) if K else 1
        arr = (_AmphOdo * max(1, K * n))()
        keep, outs = [], []
        for o, obj in enumerate(objects):
            if len(obj) != n:
                raise ValueError("every object needs the same number of parties")
            a, views = self._odo_structs(obj)
            if any(_is_dev(f) for v in views for f in v):
                raise ValueError("the batch calls take host arrays")
            keep.append(views)
            for j in range(n):
                arr[o * n + j] = a[j]
            outs.append(np.empty((a[0].nbytes // 16, 16), dtype=np.uint8))
        ff = np.full(K, -1, dtype=np.int64)
        ffp = ff.ctypes.data_as(C.POINTER(C.c_int64))
        outp = (C.c_void_p * max(1, K))(*[x.ctypes.data for x in outs])
        if masked:
            if len(secrets) != K:
                raise ValueError("one secrets array per object")
            sv = [words_view(x) for x in secrets]
            sp = (C.c_void_p * max(1, K))(*[x.ctypes.data for x in sv])
            ns = (C.c_size_t * max(1, K))(*[x.shape[0] for x in sv])
            st = lib.amph_mask_input_batch(self._h, arr, n, K, sp, ns, outp, ffp, 0)
        else:
            st = lib.amph_recombine_verify_batch(self._h, arr, n, K, outp, ffp, 0)
        self._check(st, allow_verify=True)
        return outs, ff

    def recombine_verify_batch(self, objects):
        """objects: list over secrets of recombine_verify's `odos` (host arrays).
        One launch; returns (list of (W_o, 16) secrets, int64[K] of -1 / the
        object's first failing word) -- per object what recombine_verify gives."""
        return self._batch(False, objects, None)

    def mask_input_batch(self, objects, secrets):
        """mask_input for K secrets at once; secrets[o] must hold exactly as many
        words as object o has input masks (AMPH_E_LEN otherwise)."""
        return self._batch(True, objects, secrets)

    def recombine(self, shares):
        vs = [words_view(s) for s in shares]
        flags, stream = self._mode(*vs)
        W = vs[0].shape[0]
        out = self._empty(vs[0], (W, 16))
        ptrs = (C.c_void_p * len(vs))(*[_ptr(v) for v in vs])
        self._check(lib.amph_recombine(self._h, ptrs, len(vs), W * 16, _ptr(out), flags, stream))
        return out

    def recombine_object(self, shares):
        """recombineObject exactly (client SecretShareUtil.java:70-90): each
        party's share array of its own byte length (amph_recombine_object)."""
        if len(shares) == 0:
            return np.empty((0, 16), np.uint8)
        lens = (C.c_size_t * len(shares))(*[byte_len(s) for s in shares])
        vs = [words_view(s) for s in shares]
        flags, stream = self._mode(*vs)
        W = lens[0] // 16
        out = self._empty(vs[0], (W, 16))
        ptrs = (C.c_void_p * len(vs))(*[_ptr(v) for v in vs])
        self._check(lib.amph_recombine_object(self._h, ptrs, len(vs), lens, _ptr(out), flags, stream))
        return out

    def verify(self, y, r, u, v, w):
        a = [words_view(x) for x in (y, r, u, v, w)]
        flags, stream = self._mode(*a)
        ff, ffp = self._ff(a[0])
        self._check(lib.amph_verify(self._h, *[_ptr(x) for x in a], a[0].shape[0], ffp, flags,
                                    stream), allow_verify=True)
        return self._ff_value(ff)

    def verify_message(self, y: int, r: int, u: int, v: int, w: int) -> str:
        buf = C.create_string_buffer(1024)
        n = lib.amph_verify_message(self._h, *[le16(x) for x in (y, r, u, v, w)], buf, 1024)
        if n < 0:
            raise AmphoraNativeError(-n, lib.amph_last_error().decode())
        return buf.value.decode()

    def mask_words(self, secrets16, masks16):
        s, m = words_view(secrets16), words_view(masks16)
        flags, stream = self._mode(s, m)
        out = self._empty(s, (s.shape[0], 16))
        self._check(lib.amph_mask_words(self._h, _ptr(s), _ptr(m), s.shape[0], _ptr(out), flags,
                                        stream))
        return out

    def to_gfp(self, words16):
        a = words_view(words16)
        flags, stream = self._mode(a)
        out = self._empty(a, (a.shape[0], 16))
        self._check(lib.amph_to_gfp(self._h, _ptr(a), a.shape[0], _ptr(out), flags, stream))
        return out

    def from_gfp(self, words16):
        a = words_view(words16)
        flags, stream = self._mode(a)
        out = self._empty(a, (a.shape[0], 16))
        self._check(lib.amph_from_gfp(self._h, _ptr(a), a.shape[0], _ptr(out), flags, stream))
        return out

    # -- service -------------------------------------------------------------
    def convert_share(self, masked16, tuples32, mac_key: int, use_zero_input_as_data: bool):
        m, t = words_view(masked16), words_view(tuples32, 32)
        _need(t.shape[0] >= m.shape[0], "Received more input data than available inputMasks.")
        flags, stream = self._mode(m, t)
        out = self._empty(m, (m.shape[0], 32))
        self._check(lib.amph_convert_share(self._h, _ptr(m), _ptr(t), m.shape[0],
                                           le16(mac_key % self.prime), int(use_zero_input_as_data),
                                           _ptr(out), flags, stream))
        return out

    def convert_share_json(self, text, tuples32, mac_key: int, use_zero_input_as_data: bool):
        """amph_convert_share_json: the MaskedInput "data" array text in the
        compact layout ('[' + 37-byte records + ']', one record per tuple) ->
        SecretShare.data (W, 32).  Host text (str / bytes / uint8 array): an
        offending byte or a wrong length raises AmphoraNativeError
        (AMPH_E_PARAM / AMPH_E_LEN).  Device uint8 tensor (1-D, any byte
        alignment, e.g. a view into a request body) -> (share, bad) device
        tensors, bad = AMPH_NO_FAILURE when the text held: check it before
        storing the share."""
        if isinstance(text, str):
            text = text.encode("utf-8")
        if _is_dev(text):
            a = text.reshape(-1)
            if not a.is_contiguous():
                raise ValueError("the text must be a contiguous uint8 tensor")
        elif isinstance(text, (bytes, bytearray, memoryview)):
            a = np.frombuffer(bytes(text), np.uint8)
        else:
            a = np.ascontiguousarray(text, np.uint8).reshape(-1)
        t = words_view(tuples32, 32)
        flags, stream = self._mode(a, t)
        W = t.shape[0]
        out = self._empty(t, (W, 32))
        bad, badp = self._ff(t)
        n = a.numel() if _is_dev(a) else a.size
        self._check(lib.amph_convert_share_json(self._h, _ptr(a), n, W, _ptr(t), le16(mac_key % self.prime),
                                                int(use_zero_input_as_data), _ptr(out), badp, flags, stream))
        return (out, bad) if _is_dev(a) else out

    def odo_pre(self, share_data, share_stride: int, masks32, triples96):
        sd = words_view(share_data, share_stride)
        mk, tr = words_view(masks32, 32), words_view(triples96, 96)
        W = sd.shape[0]
        # 2 input masks and 2 triples per word (OutputDeliveryService.java:102-107,177-185)
        _need(mk.shape[0] == 2 * W, "expected %d input-mask tuples, got %d" % (2 * W, mk.shape[0]))
        _need(tr.shape[0] == 2 * W, "expected %d multiplication triples, got %d" % (2 * W, tr.shape[0]))
        flags, stream = self._mode(sd, mk, tr)
        y, r, v = (self._empty(sd, (W, 16)) for _ in range(3))
        mag = self._empty(sd, (2 * W, 2, 16))
        neg = self._empty(sd, (2 * W, 2))
        self._check(lib.amph_odo_pre(self._h, _ptr(sd), share_stride, _ptr(mk), _ptr(tr), W,
                                     _ptr(y), _ptr(r), _ptr(v), _ptr(mag), _ptr(neg), flags,
                                     stream))
        return y, r, v, mag, neg

    def open_diffs(self, mags, negs):
        ms = [m if _is_dev(m) else np.ascontiguousarray(m, np.uint8) for m in mags]
        ns = [n if _is_dev(n) else np.ascontiguousarray(n, np.uint8) for n in negs]
        _need(len(ms) == len(ns) and len(ms) >= 1, "one (mag, neg) pair per party")
        n_pairs = ms[0].shape[0]
        for m, n in zip(ms, ns):  # every party opens the same 2W pairs (recombineDiffs :231-272)
            _need(tuple(m.shape) == (n_pairs, 2, 16) and tuple(n.shape) == (n_pairs, 2),
                  "party diff lists differ in length: %s / %s vs %d pairs"
                  % (tuple(m.shape), tuple(n.shape), n_pairs))
        flags, stream = self._mode(*ms, *ns)
        out = self._empty(ms[0], (n_pairs, 2, 16))
        pm = (C.c_void_p * len(ms))(*[_ptr(x) for x in ms])
        pn = (C.c_void_p * len(ns))(*[_ptr(x) for x in ns])
        self._check(lib.amph_open_diffs(self._h, pm, pn, len(ms), n_pairs, _ptr(out), flags, stream))
        return out

    def odo_post(self, opened, triples96, is_player0: bool):
        op = opened if _is_dev(opened) else np.ascontiguousarray(opened, np.uint8)
        tr = words_view(triples96, 96)
        _need(tr.shape[0] % 2 == 0 and tuple(op.shape) == (tr.shape[0], 2, 16),
              "opened values %s do not match %d triples" % (tuple(op.shape), tr.shape[0]))
        flags, stream = self._mode(op, tr)
        W = tr.shape[0] // 2
        w, u = self._empty(tr, (W, 16)), self._empty(tr, (W, 16))
        self._check(lib.amph_odo_post(self._h, _ptr(op), _ptr(tr), W, int(is_player0), _ptr(w),
                                      _ptr(u), flags, stream))
        return w, u

    def open_post(self, mags, negs, triples96, is_player0: bool):
        """open_diffs + odo_post in one launch (amph_open_post): every party's
        signed diffs + the triples -> (w, u); the opened values stay on chip."""
        ms = [m if _is_dev(m) else np.ascontiguousarray(m, np.uint8) for m in mags]
        ns = [n if _is_dev(n) else np.ascontiguousarray(n, np.uint8) for n in negs]
        tr = words_view(triples96, 96)
        _need(len(ms) == len(ns) and len(ms) >= 1, "one (mag, neg) pair per party")
        n_pairs = tr.shape[0]
        _need(n_pairs % 2 == 0, "triples must be 2 per word")
        for m, n in zip(ms, ns):
            _need(tuple(m.shape) == (n_pairs, 2, 16) and tuple(n.shape) == (n_pairs, 2),
                  "party diff lists %s / %s do not match %d triples"
                  % (tuple(m.shape), tuple(n.shape), n_pairs))
        flags, stream = self._mode(tr, *ms, *ns)
        W = n_pairs // 2
        w, u = self._empty(tr, (W, 16)), self._empty(tr, (W, 16))
        pm = (C.c_void_p * len(ms))(*[_ptr(x) for x in ms])
        pn = (C.c_void_p * len(ns))(*[_ptr(x) for x in ns])
        self._check(lib.amph_open_post(self._h, pm, pn, len(ms), _ptr(tr), W, int(is_player0), _ptr(w),
                                       _ptr(u), flags, stream))
        return w, u

    # -- K_RV / K_MASK straight from the base64 wire text ----------------------
    def _text_structs(self, texts):
        """texts: per party the five field strings (str / bytes / uint8 arrays,
        or 16-byte-aligned uint8 device tensors) in ODO order."""
        arr = (_AmphOdoB64 * len(texts))()
        keep = []
        for j, t in enumerate(texts):
            if len(t) != 5:
                raise ValueError("five base64 fields per party")
            fs = []
            for x in t:
                if isinstance(x, str):
                    x = x.encode("ascii", errors="replace")
                if isinstance(x, (bytes, bytearray, memoryview)):
                    x = np.frombuffer(bytes(x), np.uint8)
                elif not _is_dev(x):
                    x = np.ascontiguousarray(x, np.uint8).reshape(-1)
                fs.append(x)
            lens = {(f.numel() if _is_dev(f) else f.size) for f in fs}
            if len(lens) != 1:
                raise AmphoraNativeError(AMPH_E_LEN, "The provided shares must be of the same length")
            keep.extend(fs)
            arr[j] = _AmphOdoB64(*[_ptr(f) for f in fs], lens.pop())
        return arr, keep

    def recombine_verify_b64(self, texts, words: int):
        """amph_recombine_verify_b64: (canonical secrets (W, 16), first_fail,
        bad_char).  Host: first_fail / bad_char are -1 or indices (a bad
        character raises ValueError); device: int64[1] tensors."""
        arr, keep = self._text_structs(texts)
        flags, stream = self._mode(*keep)
        out = self._empty(keep[0], (words, 16))
        ff, ffp = self._ff(keep[0])
        bad, badp = self._ff(keep[0])
        st = lib.amph_recombine_verify_b64(self._h, arr, len(texts), words, _ptr(out), ffp, badp, flags, stream)
        if st == AMPH_E_PARAM and not _is_dev(keep[0]) and self._ff_value(bad) >= 0:
            raise ValueError(lib.amph_last_error().decode())
        self._check(st, allow_verify=True)
        return out, self._ff_value(ff), self._ff_value(bad)

    def mask_input_b64(self, texts, words: int, secrets16, records: bool = True, raw: bool = False):
        """amph_mask_input_b64: (masked (S, 16) or None, records (S, 24) or
        None, first_fail, bad_char)."""
        arr, keep = self._text_structs(texts)
        sv = words_view(secrets16)
        flags, stream = self._mode(sv, *keep)
        S = sv.shape[0]
        o16 = self._empty(sv, (S, 16)) if raw else None
        o24 = self._empty(sv, (S, 24)) if records else None
        ff, ffp = self._ff(sv)
        bad, badp = self._ff(sv)
        st = lib.amph_mask_input_b64(self._h, arr, len(texts), words, _ptr(sv), S,
                                     _ptr(o16) if raw else None, _ptr(o24) if records else None,
                                     ffp, badp, flags, stream)
        if self._bad_char_status(st, sv, S, words, bad):
            raise ValueError(lib.amph_last_error().decode())
        self._check(st, allow_verify=True)
        return o16, o24, self._ff_value(ff), self._ff_value(bad)

    def mask_input_json(self, texts, words: int, secrets16):
        """amph_mask_input_json: (text, first_fail, bad_char) -- mask_input_b64
        with the records written as the MaskedInput "data" array text
        ([{"value":"..."},...], 37 S + 1 characters).  Host: text is bytes;
        device: a uint8 tensor that stays on the device."""
        arr, keep = self._text_structs(texts)
        sv = words_view(secrets16)
        flags, stream = self._mode(sv, *keep)
        S = sv.shape[0]
        cap = lib.amph_masked_input_data_chars(S)
        out = self._empty(sv, (cap,))
        ff, ffp = self._ff(sv)
        bad, badp = self._ff(sv)
        st = lib.amph_mask_input_json(self._h, arr, len(texts), words, _ptr(sv), S, _ptr(out), cap,
                                      ffp, badp, flags, stream)
        if self._bad_char_status(st, sv, S, words, bad):
            raise ValueError(lib.amph_last_error().decode())
        self._check(st, allow_verify=True)
        return (out if _is_dev(sv) else out.tobytes()), self._ff_value(ff), self._ff_value(bad)

    # -- many secrets straight from their wire texts (include/amphora_wire_batch.h) --
    def wire_batch_copies(self) -> int:
        """amph_wire_batch_copies: host-device copies of the host-mode calls below."""
        return int(lib.amph_wire_batch_copies(self._h))

    def _wire_packed(self, masked, texts, word_offsets, text_offsets, secrets16, records, raw, first_fail,
                     bad_char, accumulate, status):
        arr, keep = self._text_structs(texts)
        s = words_view(secrets16) if masked else None
        flags, stream = self._mode(s, *keep)
        like = keep[0]
        K = max(0, len(word_offsets) - 1)
        if len(text_offsets) != K:
            raise ValueError("one text offset per object, one more word offset")
        T = int(word_offsets[-1]) if K else 0
        (wo, to), (first_fail, bad_char), acc = self._tables(like, K, (word_offsets, text_offsets),
                                                             (first_fail, bad_char), accumulate)
        flags |= acc
        if masked:
            _need(s.shape[0] == T, "the packed form takes one secret per input mask word")
            o16 = self._empty(like, (T, 16)) if raw else None
            o24 = self._empty(like, (T, 24)) if records else None
            st = lib.amph_mask_input_b64_packed(self._h, arr, len(texts), _ptr(wo), _ptr(to), K, _ptr(s),
                                                _ptr(o16), _ptr(o24), _ptr(first_fail), _ptr(bad_char), flags,
                                                stream)
            res = (o16, o24, first_fail, bad_char)
        else:
            out = self._empty(like, (T, 16))
            st = lib.amph_recombine_verify_b64_packed(self._h, arr, len(texts), _ptr(wo), _ptr(to), K, _ptr(out),
                                                      _ptr(first_fail), _ptr(bad_char), flags, stream)
            res = (out, first_fail, bad_char)
        return self._batch_result(st, res, bad_char, status)

    def _batch_result(self, st, res, verdict, status):
        """Per-object verdicts are the result: AMPH_E_VERIFY, and AMPH_E_PARAM
        with a bad character / offending byte reported in `verdict`, return
        them (status=True appends (status, amph_last_error)); anything else
        raises."""
        msg = lib.amph_last_error().decode() if st != AMPH_OK else ""
        if not (st == AMPH_E_PARAM and not _is_dev(verdict) and (np.asarray(verdict) >= 0).any()):
            self._check(st, allow_verify=True)
        return res + ((st, msg),) if status else res

    def _gather_objects(self, objects):
        """The gathered calls' objects[o][j] (host texts, as _text_structs) as
        one _AmphOdoB64 array [o * n + j]: (array, n, keep-alive list)."""
        K = len(objects)
        n = len(objects[0]) if K else 1
        arr = (_AmphOdoB64 * max(1, K * n))()
        keep = []
        for o, obj in enumerate(objects):
            if len(obj) != n:
                raise ValueError("every object needs the same number of parties")
            a, ks = self._text_structs(obj)
            if any(_is_dev(f) for f in ks):
                raise ValueError("the batch calls take host buffers")
            keep.append(ks)
            for j in range(n):
                arr[o * n + j] = a[j]
        return arr, n, keep

    @staticmethod
    def _dense_offsets(word_offsets, stride):
        """The default slots of a packed call's texts: object o's at the sum of
        its predecessors' stride(W) -- (offsets[K], capacity).  (A decreasing
        table gets an empty slot here and its refusal from the library.)"""
        wo = [int(x) for x in (word_offsets.cpu() if _is_dev(word_offsets) else word_offsets)]
        ends = np.cumsum([stride(max(0, b - a)) for a, b in zip(wo, wo[1:])], dtype=np.uint64)
        return np.concatenate([[0], ends]).astype(np.uint64)[:len(ends)], int(ends[-1]) if len(ends) else 0

    def recombine_verify_b64_packed(self, texts, word_offsets, text_offsets, first_fail=None, bad_char=None,
                                    accumulate=False, status=False):
        """K secrets from their base64 texts in one launch.  texts: per party
        the five field buffers, each holding every object's text at
        text_offsets[o] (multiples of 16, the same in all buffers);
        word_offsets: K + 1 word offsets of the packed outputs.  Returns
        (secrets (T, 16), first_fail[K], bad_char[K]): host -- -1 or the
        object's own index; device -- int64 tensors of AMPH_NO_FAILURE /
        index (pass them back with accumulate=True to min-combine)."""
        return self._wire_packed(False, texts, word_offsets, text_offsets, None, False, False, first_fail,
                                 bad_char, accumulate, status)

    def mask_input_b64_packed(self, texts, word_offsets, text_offsets, secrets16, records=True, raw=False,
                              first_fail=None, bad_char=None, accumulate=False, status=False):
        """recombine_verify_b64_packed over Input Mask ODO texts fused with
        maskInput, one secret per mask word: (masked (T, 16) or None, records
        (T, 24) or None, first_fail[K], bad_char[K])."""
        return self._wire_packed(True, texts, word_offsets, text_offsets, secrets16, records, raw, first_fail,
                                 bad_char, accumulate, status)

    def _wire_batch(self, masked, objects, words, secrets, records, raw, status):
        K = len(objects)
        arr, n, keep = self._gather_objects(objects)
        wd = (C.c_size_t * max(1, K))(*[int(w) for w in words])
        ff = np.full(K, -1, dtype=np.int64)
        bad = np.full(K, -1, dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        ptrs = lambda xs: (C.c_void_p * max(1, K))(*[x.ctypes.data for x in xs]) if xs is not None else None
        if masked:
            if len(secrets) != K:
                raise ValueError("one secrets array per object")
            sv = [words_view(x) for x in secrets]
            for o in range(K):
                _need(sv[o].shape[0] == int(words[o]), "object %d: one secret per input mask word" % o)
            o16 = [np.empty((int(w), 16), np.uint8) for w in words] if raw else None
            o24 = [np.empty((int(w), 24), np.uint8) for w in words] if records else None
            st = lib.amph_mask_input_b64_batch(self._h, arr, n, K, wd, ptrs(sv), ptrs(o16), ptrs(o24),
                                               ff.ctypes.data_as(i64p), bad.ctypes.data_as(i64p), 0)
            res = (o16, o24, ff, bad)
        else:
            outs = [np.empty((int(w), 16), np.uint8) for w in words]
            st = lib.amph_recombine_verify_b64_batch(self._h, arr, n, K, wd, ptrs(outs), ff.ctypes.data_as(i64p),
                                                     bad.ctypes.data_as(i64p), 0)
            res = (outs, ff, bad)
        return self._batch_result(st, res, bad, status)

    def recombine_verify_b64_batch(self, objects, words, status=False):
        """objects: list over secrets of recombine_verify_b64's `texts` (host
        strings / bytes), words[o] each object's word count.  One launch;
        returns (list of (W_o, 16) secrets, first_fail[K], bad_char[K]) -- per
        object what recombine_verify_b64 gives."""
        return self._wire_batch(False, objects, words, None, False, False, status)

    def mask_input_b64_batch(self, objects, words, secrets, records=True, raw=False, status=False):
        """mask_input_b64 for K secrets at once, secrets[o] of exactly words[o]
        words: (list of masked (W_o, 16) or None, list of records (W_o, 24) or
        None, first_fail[K], bad_char[K])."""
        return self._wire_batch(True, objects, words, secrets, records, raw, status)

    # -- many MaskedInput uploads per launch (include/amphora_upload_batch.h) --------
    def upload_batch_copies(self) -> int:
        """amph_upload_batch_copies: host-device copies of the host-mode calls below."""
        return int(lib.amph_upload_batch_copies(self._h))

    @staticmethod
    def _bytes_view(x):
        if isinstance(x, str):
            x = x.encode("utf-8")
        if _is_dev(x):
            a = x.reshape(-1)
            if not a.is_contiguous():
                raise ValueError("the text must be a contiguous uint8 tensor")
            return a
        if isinstance(x, (bytes, bytearray, memoryview)):
            return np.frombuffer(bytes(x), np.uint8)
        return np.ascontiguousarray(x, np.uint8).reshape(-1)

    def _tables(self, like, K, tables, verdicts, accumulate):
        """The offset tables and verdict arrays of a packed batch call where
        `like` lives: (tables, verdicts, extra flags)."""
        if _is_dev(like):
            import torch
            tables = [x if _is_dev(x) else torch.as_tensor(np.ascontiguousarray(x, np.uint64).view(np.int64))
                      .to(like.device) for x in tables]
            out = []
            for v in verdicts:
                if v is None:
                    v = torch.empty(K, dtype=torch.int64, device=like.device)
                    accumulate = False
                elif v.numel() != K or v.dtype != torch.int64 or not v.is_cuda:
                    raise ValueError("verdict arrays must be int64 device tensors with one entry per object")
                out.append(v)
            return tables, out, (AMPH_F_ACCUMULATE if accumulate else 0)
        return ([np.ascontiguousarray(x, dtype=np.uint64) for x in tables],
                [np.full(K, -1, dtype=np.int64) for _ in verdicts], 0)

    def convert_share_json_packed(self, texts, word_offsets, text_offsets, tuples32, mac_key: int,
                                  use_zero_input_as_data: bool, out=None, bad_index=None, accumulate=False,
                                  status=False):
        """amph_convert_share_json_packed: K MaskedInput "data" array texts ->
        K shares in one launch.  texts: one buffer (bytes / uint8 array, or a
        1-D uint8 device tensor) holding object o's text at text_offsets[o]
        (any alignment); tuples32 (T, 32) packed on word_offsets[K + 1].
        Returns (shares (T, 32), bad_index[K]): host -- -1 or the offending
        byte's offset inside the object's own text; device -- int64 tensor of
        AMPH_NO_FAILURE / offset."""
        a, t = self._bytes_view(texts), words_view(tuples32, 32)
        flags, stream = self._mode(a, t)
        n = a.numel() if _is_dev(a) else a.size
        K = max(0, len(word_offsets) - 1)
        if len(text_offsets) != K:
            raise ValueError("one text offset per object, one more word offset")
        (wo, to), (bad,), acc = self._tables(a, K, (word_offsets, text_offsets), (bad_index,), accumulate)
        out = self._out(t, (t.shape[0], 32), out)
        st = lib.amph_convert_share_json_packed(self._h, _ptr(a), n, _ptr(wo), _ptr(to), K, _ptr(t),
                                                le16(mac_key % self.prime), int(use_zero_input_as_data), _ptr(out),
                                                _ptr(bad), flags | acc, stream)
        return self._batch_result(st, (out, bad), bad, status)

    def convert_share_json_batch(self, texts, tuples, mac_key: int, use_zero_input_as_data: bool, status=False):
        """amph_convert_share_json_batch: texts[o] (str / bytes) with
        tuples[o] ((W_o, 32)), host memory.  Returns (list of (W_o, 32)
        shares, bad_index[K]) -- per object what convert_share_json gives."""
        K = len(texts)
        if len(tuples) != K:
            raise ValueError("one tuple array per text")
        tv = [self._bytes_view(x) for x in texts]
        tu = [words_view(x, 32) for x in tuples]
        outs = [np.empty((x.shape[0], 32), np.uint8) for x in tu]
        bad = np.full(K, -1, dtype=np.int64)
        szs = lambda xs: (C.c_size_t * max(1, K))(*xs)  # noqa: E731
        ptrs = lambda xs: (C.c_void_p * max(1, K))(*[x.ctypes.data for x in xs])  # noqa: E731
        st = lib.amph_convert_share_json_batch(self._h, ptrs(tv), szs([x.size for x in tv]),
                                               szs([x.shape[0] for x in tu]), K, ptrs(tu),
                                               le16(mac_key % self.prime), int(use_zero_input_as_data), ptrs(outs),
                                               bad.ctypes.data_as(C.POINTER(C.c_int64)), 0)
        return self._batch_result(st, (outs, bad), bad, status)

    def mask_input_json_packed(self, texts, word_offsets, text_offsets, secrets16, out_text_offsets=None,
                               out_text=None, first_fail=None, bad_char=None, accumulate=False, status=False):
        """amph_mask_input_json_packed: mask_input_b64_packed with every
        object's records written as its framed "data" array text.  Object o's
        text goes to out_text[out_text_offsets[o]:] (multiples of 16; default:
        the dense layout of upload_slot_chars strides in a fresh buffer).
        Returns (out_text uint8 buffer, out_text_offsets, first_fail[K],
        bad_char[K])."""
        arr, keep = self._text_structs(texts)
        s = words_view(secrets16)
        flags, stream = self._mode(s, *keep)
        like = keep[0]
        K = max(0, len(word_offsets) - 1)
        if len(text_offsets) != K:
            raise ValueError("one text offset per object, one more word offset")
        cap = None
        if out_text_offsets is None:
            out_text_offsets, cap = self._dense_offsets(word_offsets, upload_slot_chars)
        if out_text is None:
            if cap is None:
                raise ValueError("out_text_offsets of the caller's need the caller's out_text")
            out_text = self._empty(like, (max(16, cap),))
        cap = out_text.numel() if _is_dev(out_text) else out_text.size
        (wo, to, oo), (ff, bad), acc = self._tables(like, K, (word_offsets, text_offsets, out_text_offsets),
                                                    (first_fail, bad_char), accumulate)
        st = lib.amph_mask_input_json_packed(self._h, arr, len(texts), _ptr(wo), _ptr(to), K, _ptr(s),
                                             _ptr(out_text), cap, _ptr(oo), _ptr(ff), _ptr(bad), flags | acc, stream)
        return self._batch_result(st, (out_text, oo, ff, bad), bad, status)

    def mask_input_json_batch(self, objects, words, secrets, status=False):
        """amph_mask_input_json_batch: mask_input_json for K secrets at once
        (host strings / bytes): (list of K texts as bytes, first_fail[K],
        bad_char[K])."""
        K = len(objects)
        arr, n, keep = self._gather_objects(objects)
        if len(secrets) != K:
            raise ValueError("one secrets array per object")
        sv = [words_view(x) for x in secrets]
        for o in range(K):
            _need(sv[o].shape[0] == int(words[o]), "object %d: one secret per input mask word" % o)
        wd = (C.c_size_t * max(1, K))(*[int(w) for w in words])
        outs = [np.empty(masked_input_data_chars(int(w)), np.uint8) for w in words]
        ff, bad = np.full(K, -1, dtype=np.int64), np.full(K, -1, dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        ptrs = lambda xs: (C.c_void_p * max(1, K))(*[x.ctypes.data for x in xs])  # noqa: E731
        st = lib.amph_mask_input_json_batch(self._h, arr, n, K, wd, ptrs(sv), ptrs(outs), ff.ctypes.data_as(i64p),
                                            bad.ctypes.data_as(i64p), 0)
        return self._batch_result(st, ([x.tobytes() for x in outs], ff, bad), bad, status)

    # -- many Output Delivery responses per launch (include/amphora_respond_batch.h) --
    def respond_batch_copies(self) -> int:
        """amph_respond_batch_copies: host-device copies of the host-mode calls below."""
        return int(lib.amph_respond_batch_copies(self._h))

    def odo_fields_b64_packed(self, fields5, word_offsets, text_offsets=None, out=None, reject=None):
        """amph_odo_fields_b64_packed: K objects' five base64 field texts in one
        launch.  fields5: the five packed word arrays ((T, 16) each, host arrays
        or device tensors) in ODO order, the objects on word_offsets[K + 1];
        object o's text of every field goes to text_offsets[o] of that field's
        buffer (multiples of 16; default: the dense layout of wire_slot_chars
        strides).  out: five uint8 buffers of one length (default: fresh ones
        that end with the last slot); bytes outside the texts are not written.
        reject: None or one int64 per object -- host: >= 0 rejects, device
        tensor: != AMPH_NO_FAILURE rejects -- a rejected object's texts start
        "!!!!".  Returns (the five buffers, text_offsets): what
        recombine_verify_b64_packed takes as one party's texts and table."""
        if len(fields5) != 5:
            raise ValueError("five ODO fields")
        lens = {byte_len(f) for f in fields5}
        if len(lens) != 1:
            raise AmphoraNativeError(AMPH_E_LEN, "The provided shares must be of the same length")
        nbytes = lens.pop()
        fs = [f if _is_dev(f) else np.ascontiguousarray(f, np.uint8).reshape(-1) for f in fields5]
        flags, stream = self._mode(*fs)
        like = fs[0]
        K = max(0, len(word_offsets) - 1)
        cap = None
        if text_offsets is None:
            text_offsets, cap = self._dense_offsets(word_offsets, wire_slot_chars)
        if len(text_offsets) != K:
            raise ValueError("one text offset per object, one more word offset")
        if out is None:
            if cap is None:
                raise ValueError("text_offsets of the caller's need the caller's out buffers")
            out = [self._empty(like, (max(16, cap),)) for _ in range(5)]
        if len(out) != 5 or any(_is_dev(b) != _is_dev(like) for b in out):
            raise ValueError("out: five buffers that live where the inputs live")
        caps = {(b.numel() if _is_dev(b) else b.size) for b in out}
        if len(caps) != 1:
            raise ValueError("the five output buffers must have one length")
        (wo, to), _, _ = self._tables(like, K, (word_offsets, text_offsets), (), False)
        if _is_dev(like):
            import torch
            if reject is not None and not (_is_dev(reject) and reject.dtype == torch.int64 and reject.numel() == K):
                raise ValueError("reject must be an int64 device tensor with one entry per object")
            rj = reject
        else:
            rj = None if reject is None else np.ascontiguousarray(reject, dtype=np.int64)
            if rj is not None and rj.size != K:
                raise ValueError("one reject word per object")
        odo = _AmphOdo(*[_ptr(f) for f in fs], nbytes)
        ob = _AmphOdoB64Out(*[_ptr(b) for b in out], caps.pop())
        self._check(lib.amph_odo_fields_b64_packed(self._h, C.byref(odo), _ptr(wo), _ptr(to), K, C.byref(ob),
                                                   _ptr(rj), flags, stream))
        return out, to

    def odo_fields_b64_batch(self, list_of_fields5, reject=None):
        """amph_odo_fields_b64_batch: fields5 (host word arrays) per object ->
        per object its five base64 texts as bytes, one launch for all."""
        K = len(list_of_fields5)
        arr = (_AmphOdo * max(1, K))()
        keep, outs = [], []
        for o, f5 in enumerate(list_of_fields5):
            if len(f5) != 5:
                raise ValueError("five ODO fields per object")
            lens = {byte_len(f) for f in f5}
            if len(lens) != 1:
                raise AmphoraNativeError(AMPH_E_LEN, "The provided shares must be of the same length")
            fs = [np.ascontiguousarray(f, np.uint8).reshape(-1) for f in f5]
            if any(_is_dev(f) for f in f5):
                raise ValueError("the batch calls take host buffers")
            keep.append(fs)
            nbytes = lens.pop()
            arr[o] = _AmphOdo(*[_ptr(f) for f in fs], nbytes)
            outs.extend(np.empty(max(1, wire_text_chars(nbytes // 16)), np.uint8) for _ in range(5))
        rj = None if reject is None else np.ascontiguousarray(reject, dtype=np.int64)
        if rj is not None and rj.size != K:
            raise ValueError("one reject word per object")
        po = (C.c_void_p * max(1, 5 * K))(*[x.ctypes.data for x in outs])
        self._check(lib.amph_odo_fields_b64_batch(self._h, arr, K, po, _ptr(rj), 0))
        return [[outs[5 * o + k][:wire_text_chars(arr[o].nbytes // 16)].tobytes() for k in range(5)]
                for o in range(K)]

    # -- wire codec (base64 as Jackson writes byte[]) ---------------------------
    def base64_encode(self, data) -> bytes:
        """bytes / uint8 array -> base64 ASCII (bytes); device tensor -> device tensor."""
        a = data if _is_dev(data) else np.frombuffer(bytes(data), np.uint8) \
            if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8).reshape(-1)
        n = a.numel() if _is_dev(a) else a.size
        flags, stream = self._mode(a)
        out = self._empty(a, (4 * ((n + 2) // 3),))
        self._check(lib.amph_base64_encode(self._h, _ptr(a), n, _ptr(out), flags, stream))
        return out if _is_dev(a) else out.tobytes()

    def base64_decode(self, text, nbytes: int | None = None) -> bytes:
        """base64 ASCII (str / bytes / uint8 array) -> bytes; raises ValueError on
        an illegal character or a length not divisible by 4.  Device text ->
        (uint8 tensor, bad-index word); with nbytes (the decoded length the
        caller expects, e.g. 16 per word of an ODO field) the call is fully
        asynchronous (no read-back of the padding to size the output).
        nbytes must then EQUAL the text's decoded length, 3 n / 4 minus its
        '=' padding: it is only range-checked here (the padding is on the
        device), and a wrong value returns a slice that cuts decoded bytes
        (too small) or ends in bytes the kernel never wrote (too large)."""
        if isinstance(text, str):
            text = text.encode("ascii", errors="replace")
        a = text if _is_dev(text) else np.frombuffer(bytes(text), np.uint8) \
            if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, np.uint8).reshape(-1)
        n = a.numel() if _is_dev(a) else a.size
        flags, stream = self._mode(a)
        out = self._empty(a, (3 * n // 4,))
        ob = C.c_size_t(0)
        async_dev = _is_dev(a) and nbytes is not None
        if async_dev and not (n % 4 == 0 and 3 * n // 4 - 2 <= nbytes <= 3 * n // 4):
            raise ValueError("nbytes %d does not fit a %d-character text" % (nbytes, n))
        bad, badp = self._ff(a)
        st = lib.amph_base64_decode(self._h, _ptr(a), n, _ptr(out), None if async_dev else C.byref(ob), badp,
                                    flags, stream)
        if st in (AMPH_E_PARAM, AMPH_E_LEN):
            raise ValueError(lib.amph_last_error().decode())
        self._check(st)
        if _is_dev(a):
            return out[: nbytes if async_dev else ob.value], bad
        return out[: ob.value].tobytes()

    def base64_encode_words(self, words16):
        w = words_view(words16)
        flags, stream = self._mode(w)
        out = self._empty(w, (w.shape[0], 24))
        self._check(lib.amph_base64_encode_words(self._h, _ptr(w), w.shape[0], _ptr(out), flags, stream))
        return out

    def base64_decode_words(self, records24):
        r = words_view(records24, 24)
        flags, stream = self._mode(r)
        out = self._empty(r, (r.shape[0], 16))
        bad, badp = self._ff(r)
        st = lib.amph_base64_decode_words(self._h, _ptr(r), r.shape[0], _ptr(out), badp, flags, stream)
        if st == AMPH_E_PARAM and not _is_dev(r):
            raise ValueError(lib.amph_last_error().decode())
        self._check(st)
        return out if not _is_dev(r) else (out, bad)

    # -- Beaver open exchange (MultiplicationExchangeObject.interimValues) ------
    def exchange_encode(self, mag, neg):
        """Signed diffs (amph_odo_pre layout: mag (P, 2, 16), neg (P, 2)) -> the
        FactorPair JSON array text.  Host arrays -> bytes; device tensors ->
        (uint8 tensor with capacity amph_exchange_max_chars(P), length tensor)."""
        m = mag if _is_dev(mag) else np.ascontiguousarray(mag, np.uint8)
        g = neg if _is_dev(neg) else np.ascontiguousarray(neg, np.uint8)
        flags, stream = self._mode(m, g)
        P = m.shape[0]
        cap = lib.amph_exchange_max_chars(P)
        out = self._empty(m, (cap,))
        if _is_dev(m):
            import torch
            n = torch.empty(1, dtype=torch.int64, device=m.device)
            self._check(lib.amph_exchange_encode(self._h, _ptr(m), _ptr(g), P, _ptr(out), cap,
                                                 C.c_void_p(n.data_ptr()), flags, stream))
            return out, n
        n = C.c_uint64(0)
        self._check(lib.amph_exchange_encode(self._h, _ptr(m), _ptr(g), P, _ptr(out), cap,
                                             C.addressof(n), flags, stream))
        return out[: n.value].tobytes()

    def exchange_decode(self, text, npairs: int):
        """FactorPair JSON array text -> (mag (P, 2, 16), neg (P, 2)); raises
        ValueError on a malformed token or a count other than npairs.  Device
        uint8 tensor in -> (mag, neg, bad) device tensors, bad = AMPH_NO_FAILURE
        when clean."""
        if isinstance(text, str):
            text = text.encode("utf-8")
        a = text if _is_dev(text) else np.frombuffer(bytes(text), np.uint8)
        n = a.numel() if _is_dev(a) else a.size
        flags, stream = self._mode(a)
        mag = self._empty(a, (npairs, 2, 16))
        neg = self._empty(a, (npairs, 2))
        bad, badp = self._ff(a)
        st = lib.amph_exchange_decode(self._h, _ptr(a), n, npairs, _ptr(mag), _ptr(neg), badp, flags,
                                      stream)
        if st in (AMPH_E_PARAM, AMPH_E_LEN) and not _is_dev(a):
            raise ValueError(lib.amph_last_error().decode())
        self._check(st)
        return (mag, neg) if not _is_dev(a) else (mag, neg, bad)

    # -- many requests' exchange texts per call (include/amphora_exchange_batch.h) --
    def exchange_batch_copies(self) -> int:
        """amph_exchange_batch_copies: host-device copies of the host-mode calls below."""
        return int(lib.amph_exchange_batch_copies(self._h))

    def _exchange_result(self, st, res, verdict, status):
        """The decode's verdicts are its result: AMPH_E_PARAM / AMPH_E_LEN with
        an offset reported in `verdict` return them (status=True appends
        (status, amph_last_error)); anything else raises."""
        msg = lib.amph_last_error().decode() if st != AMPH_OK else ""
        if not (st in (AMPH_E_PARAM, AMPH_E_LEN) and not _is_dev(verdict) and (np.asarray(verdict) >= 0).any()):
            self._check(st)
        return res + ((st, msg),) if status else res

    def exchange_encode_packed(self, mag, neg, pair_offsets, text_offsets=None, out=None, out_lens=None):
        """amph_exchange_encode_packed: K objects' FactorPair array texts from
        one call.  mag (T, 2, 16) / neg (T, 2): the objects' diffs (amph_odo_pre's
        layout, host arrays or device tensors) on pair_offsets[K + 1]; object o's
        text goes to out[text_offsets[o]:] (multiples of
        AMPH_EXCHANGE_SLOT_ALIGN; default: the dense layout of
        exchange_slot_chars strides in a fresh buffer).  Bytes outside the texts
        are not written.  Returns (out, text_offsets, out_lens): what
        exchange_decode_packed takes as texts, text_offsets and text_lens."""
        m = mag if _is_dev(mag) else np.ascontiguousarray(mag, np.uint8)
        g = neg if _is_dev(neg) else np.ascontiguousarray(neg, np.uint8)
        flags, stream = self._mode(m, g)
        T = byte_len(m) // 32
        K = max(0, len(pair_offsets) - 1)
        cap = None
        if text_offsets is None:
            text_offsets, cap = self._dense_offsets(pair_offsets, exchange_slot_chars)
        if len(text_offsets) != K:
            raise ValueError("one text offset per object, one more pair offset")
        if out is None:
            if cap is None:
                raise ValueError("text_offsets of the caller's need the caller's out buffer")
            out = self._empty(m, (max(16, cap),))
        if _is_dev(out) != _is_dev(m):
            raise ValueError("out must live where the diffs live")
        cap = out.numel() if _is_dev(out) else out.size
        (po, to), _, _ = self._tables(m, K, (pair_offsets, text_offsets), (), False)
        if out_lens is None:
            out_lens = self._empty(m, (max(1, K),), "int64")[:K] if _is_dev(m) else np.zeros(K, np.uint64)
        st = lib.amph_exchange_encode_packed(self._h, _ptr(m), _ptr(g), T, _ptr(po), _ptr(to), K, _ptr(out), cap,
                                             _ptr(out_lens), flags, stream)
        self._check(st)
        return out, to, out_lens

    def exchange_encode_batch(self, mags, negs, out_caps=None, status=False):
        """amph_exchange_encode_batch: per object its diffs (host arrays) ->
        per object its text as bytes, one call for all.  out_caps (testing the
        capacity rule): a text longer than its out_caps[o] is left out (None in
        its place) and the call's AMPH_E_LEN returned with status=True."""
        K = len(mags)
        if len(negs) != K:
            raise ValueError("one sign array per magnitude array")
        ms = [np.ascontiguousarray(x, np.uint8).reshape(-1) for x in mags]
        gs = [np.ascontiguousarray(x, np.uint8).reshape(-1) for x in negs]
        nps = [x.size // 32 for x in ms]
        caps = [int(lib.amph_exchange_max_chars(n)) for n in nps] if out_caps is None else [int(c) for c in out_caps]
        outs = [np.zeros(max(1, c), np.uint8) for c in caps]
        lens = np.zeros(max(1, K), np.uint64)
        szs = lambda xs: (C.c_size_t * max(1, K))(*xs)  # noqa: E731
        ptrs = lambda xs: (C.c_void_p * max(1, K))(*[x.ctypes.data for x in xs])  # noqa: E731
        st = lib.amph_exchange_encode_batch(self._h, ptrs(ms), ptrs(gs), szs(nps), K, ptrs(outs), szs(caps),
                                            lens.ctypes.data, 0)
        msg = lib.amph_last_error().decode() if st != AMPH_OK else ""
        if not (st == AMPH_E_LEN and status):
            self._check(st)
        texts = [outs[o][:int(lens[o])].tobytes() if int(lens[o]) <= caps[o] else None for o in range(K)]
        return (texts, lens[:K], (st, msg)) if status else texts

    def exchange_decode_packed(self, texts, pair_offsets, text_offsets, text_lens, bad_index=None, accumulate=False,
                               status=False, npairs_total=None):
        """amph_exchange_decode_packed: K texts in one buffer (uint8 array /
        bytes, or a 1-D uint8 device tensor), object o's text_lens[o] characters
        at text_offsets[o], expected to hold pair_offsets[o + 1] -
        pair_offsets[o] pairs.  Returns (mag (T, 2, 16), neg (T, 2),
        bad_index[K]): host -- -1, the offending byte's offset inside the
        object's own text, or its length on a count mismatch; device -- int64
        tensor of AMPH_NO_FAILURE / offset.  A faulty object's own rows are
        unspecified.  npairs_total: pair_offsets[K], which sizes the outputs; a
        host table gives it, a device table is never read here (the call stays
        asynchronous), so it must come with one."""
        a = self._bytes_view(texts)
        flags, stream = self._mode(a)
        n = a.numel() if _is_dev(a) else a.size
        K = max(0, len(pair_offsets) - 1)
        if len(text_offsets) != K or len(text_lens) != K:
            raise ValueError("one text offset and length per object, one more pair offset")
        if npairs_total is None:
            if _is_dev(pair_offsets):
                raise ValueError("a device pair table needs npairs_total: the table is not read on the host")
            npairs_total = int(pair_offsets[-1]) if K else 0
        T = int(npairs_total)
        (po, to, tl), (bad,), acc = self._tables(a, K, (pair_offsets, text_offsets, text_lens), (bad_index,),
                                                 accumulate)
        mag = self._empty(a, (T, 2, 16))
        neg = self._empty(a, (T, 2))
        st = lib.amph_exchange_decode_packed(self._h, _ptr(a), n, _ptr(po), _ptr(to), _ptr(tl), K, T, _ptr(mag),
                                             _ptr(neg), _ptr(bad), flags | acc, stream)
        return self._exchange_result(st, (mag, neg, bad), bad, status)

    def exchange_decode_batch(self, texts, npairs, status=False):
        """amph_exchange_decode_batch: texts[o] (str / bytes) expected to hold
        npairs[o] pairs -> (list of (mag (P_o, 2, 16), neg (P_o, 2)),
        bad_index[K]) -- per object what exchange_decode gives."""
        K = len(texts)
        if len(npairs) != K:
            raise ValueError("one pair count per text")
        tv = [self._bytes_view(x) for x in texts]
        if any(_is_dev(x) for x in tv):
            raise ValueError("the batch calls take host buffers")
        mags = [np.zeros((int(p), 2, 16), np.uint8) for p in npairs]
        negs = [np.zeros((int(p), 2), np.uint8) for p in npairs]
        bad = np.full(K, -1, dtype=np.int64)
        szs = lambda xs: (C.c_size_t * max(1, K))(*xs)  # noqa: E731
        ptrs = lambda xs: (C.c_void_p * max(1, K))(*[x.ctypes.data for x in xs])  # noqa: E731
        st = lib.amph_exchange_decode_batch(self._h, ptrs(tv), szs([x.size for x in tv]),
                                            szs([int(p) for p in npairs]), K, ptrs(mags), ptrs(negs),
                                            bad.ctypes.data_as(C.POINTER(C.c_int64)), 0)
        return self._exchange_result(st, (list(zip(mags, negs)), bad), bad, status)

    # -- one party's Output Delivery, device-resident between steps ------------
    def party_begin(self, share_data, share_stride: int, masks32, triples96, n_parties: int,
                    want_yrv: bool = True) -> "PartySession":
        """amph_party_begin from host buffers: the tuples in, (y, r, v) out
        (unless want_yrv is False), this party's interimValues text kept on
        the device (PartySession.text())."""
        sd = words_view(share_data, share_stride)
        mk, tr = words_view(masks32, 32), words_view(triples96, 96)
        W = sd.shape[0]
        _need(mk.shape[0] == 2 * W, "expected %d input-mask tuples, got %d" % (2 * W, mk.shape[0]))
        _need(tr.shape[0] == 2 * W, "expected %d multiplication triples, got %d" % (2 * W, tr.shape[0]))
        yrv = tuple(np.empty((W, 16), np.uint8) for _ in range(3)) if want_yrv else (None, None, None)
        h = C.c_void_p()
        self._check(lib.amph_party_begin(self._h, _ptr(sd), share_stride, _ptr(mk), _ptr(tr), W, n_parties,
                                         *[_ptr(x) for x in yrv], C.byref(h)))
        return PartySession(self, h, W, n_parties, yrv)

    def party_begin_dev(self, share_data, share_stride: int, masks32, triples96, n_parties: int,
                        want_yrv: bool = False) -> "PartySessionDev":
        """amph_party_begin_dev on torch device tensors (used in place; the
        triples must stay unchanged until finish), asynchronous on torch's
        current stream."""
        import torch
        W = share_data.shape[0]
        _need(share_data.is_cuda and masks32.is_cuda and triples96.is_cuda, "device tensors expected")
        _need(share_data.numel() == W * share_stride, "share data: %d words of %d bytes" % (W, share_stride))
        _need(masks32.numel() == 64 * W, "expected %d input-mask tuples" % (2 * W))
        _need(triples96.numel() == 192 * W, "expected %d multiplication triples" % (2 * W))
        yrv = tuple(torch.empty((W, 16), dtype=torch.uint8, device=share_data.device) for _ in range(3)) \
            if want_yrv else (None, None, None)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        h = C.c_void_p()
        self._check(lib.amph_party_begin_dev(self._h, _ptr(share_data), share_stride, _ptr(masks32),
                                             _ptr(triples96), W, n_parties, *[_ptr(x) for x in yrv], stream,
                                             C.byref(h)))
        return PartySessionDev(self, h, W, n_parties, yrv, (share_data, masks32, triples96))

    # -- many requests of one party in one device-resident session -------------
    def parties_begin(self, share_data, share_stride: int, masks32, triples96, word_offsets, n_parties: int,
                      want_yrv: bool = True) -> "PartySessions":
        """amph_parties_begin from host buffers: the packed tuples of K
        requests (request o = words [word_offsets[o], word_offsets[o + 1])) in,
        the packed (y, r, v) out (unless want_yrv is False), this party's K
        interimValues texts kept on the device (PartySessions.texts())."""
        wo = np.ascontiguousarray(word_offsets, dtype=np.uint64)
        _need(wo.ndim == 1 and wo.size >= 1, "word_offsets: one entry per object and the total")
        sd = words_view(share_data, share_stride)
        mk, tr = words_view(masks32, 32), words_view(triples96, 96)
        T = sd.shape[0]
        _need(int(wo[-1]) == T, "word_offsets must end at the %d words of the share data" % T)
        _need(mk.shape[0] == 2 * T, "expected %d input-mask tuples, got %d" % (2 * T, mk.shape[0]))
        _need(tr.shape[0] == 2 * T, "expected %d multiplication triples, got %d" % (2 * T, tr.shape[0]))
        yrv = tuple(np.empty((T, 16), np.uint8) for _ in range(3)) if want_yrv else (None, None, None)
        h = C.c_void_p()
        self._check(lib.amph_parties_begin(self._h, _ptr(sd), share_stride, _ptr(mk), _ptr(tr), _ptr(wo),
                                           wo.size - 1, n_parties, *[_ptr(x) for x in yrv], C.byref(h)))
        return PartySessions(self, h, wo, n_parties, yrv)

    def parties_begin_dev(self, share_data, share_stride: int, masks32, triples96, word_offsets, n_parties: int,
                          want_yrv: bool = False) -> "PartySessionsDev":
        """amph_parties_begin_dev on torch device tensors (used in place; the
        triples must stay unchanged until finish); word_offsets is a host
        array.  Asynchronous on torch's current stream."""
        import torch
        wo = np.ascontiguousarray(word_offsets, dtype=np.uint64)
        _need(wo.ndim == 1 and wo.size >= 1, "word_offsets: one entry per object and the total")
        T = int(wo[-1])
        _need(share_data.is_cuda and masks32.is_cuda and triples96.is_cuda, "device tensors expected")
        _need(share_data.numel() == T * share_stride, "share data: %d words of %d bytes" % (T, share_stride))
        _need(masks32.numel() == 64 * T, "expected %d input-mask tuples" % (2 * T))
        _need(triples96.numel() == 192 * T, "expected %d multiplication triples" % (2 * T))
        yrv = tuple(torch.empty((T, 16), dtype=torch.uint8, device=share_data.device) for _ in range(3)) \
            if want_yrv else (None, None, None)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        h = C.c_void_p()
        self._check(lib.amph_parties_begin_dev(self._h, _ptr(share_data), share_stride, _ptr(masks32),
                                               _ptr(triples96), _ptr(wo), wo.size - 1, n_parties,
                                               *[_ptr(x) for x in yrv], stream, C.byref(h)))
        return PartySessionsDev(self, h, wo, n_parties, yrv, (share_data, masks32, triples96))

    # -- the client side as a session (include/amphora_client_session.h) -------
    def client_begin(self, words: int, n_parties: int) -> "ClientSession":
        """amph_client_begin: a host-mode session that takes each party's five
        base64 texts as they arrive (ClientSession.party) and finishes from
        the running sums."""
        h = C.c_void_p()
        self._check(lib.amph_client_begin(self._h, words, n_parties, C.byref(h)))
        return ClientSession(self, h, words, n_parties, None)

    def client_begin_dev(self, words: int, n_parties: int, stream=None) -> "ClientSession":
        """amph_client_begin_dev: texts, secrets, outputs and verdict words are
        torch device tensors, every call asynchronous on the ONE stream of the
        session (`stream`: a torch stream; torch's current stream when None)."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        h = C.c_void_p()
        self._check(lib.amph_client_begin_dev(self._h, words, n_parties, C.c_void_p(stream.cuda_stream), C.byref(h)))
        return ClientSession(self, h, words, n_parties, stream)

    # -- the client side as a session for K secrets (include/amphora_client_batch.h) --
    def clients_begin(self, word_offsets, n_parties: int) -> "ClientSessions":
        """amph_clients_begin: a host-mode session for K secrets (secret o =
        words [word_offsets[o], word_offsets[o + 1])) that takes each party's
        five slotted field buffers as they arrive (ClientSessions.party /
        party_texts) and finishes from the running sums, a verdict per secret."""
        wo = np.ascontiguousarray(word_offsets, dtype=np.uint64)
        _need(wo.ndim == 1 and wo.size >= 1, "word_offsets: one entry per object and the total")
        h = C.c_void_p()
        self._check(lib.amph_clients_begin(self._h, _ptr(wo), wo.size - 1, n_parties, C.byref(h)))
        return ClientSessions(self, h, wo, n_parties, None)

    def clients_begin_dev(self, word_offsets, n_parties: int, stream=None) -> "ClientSessions":
        """amph_clients_begin_dev: word_offsets is a host array; texts,
        secrets, outputs and verdict arrays are torch device tensors, every
        call asynchronous on the ONE stream of the session (`stream`: a torch
        stream; torch's current stream when None)."""
        import torch
        wo = np.ascontiguousarray(word_offsets, dtype=np.uint64)
        _need(wo.ndim == 1 and wo.size >= 1, "word_offsets: one entry per object and the total")
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        h = C.c_void_p()
        self._check(lib.amph_clients_begin_dev(self._h, _ptr(wo), wo.size - 1, n_parties,
                                               C.c_void_p(stream.cuda_stream), C.byref(h)))
        return ClientSessions(self, h, wo, n_parties, stream)

    def clients_copies(self) -> int:
        """amph_clients_copies: host-device copies of the host-mode ClientSessions calls."""
        return int(lib.amph_clients_copies(self._h))

    # -- synthetic device inputs (bench / tests) --------------------------------
    def synth_odos(self, seed: int, n: int, words: int, fault_index: int = -1,
                   noncanon_permille: int = 0, with_plain: bool = False, buf=None):
        """Returns (odos, buffer, plain_y): a (5, n, W, 16) uint8 device
        tensor, the per-party (y, r, v, w, u) views of it, optional secrets.
        `buf`: generate into the caller's (5, n, W, 16) device tensor."""
        import torch
        if buf is None:
            buf = torch.empty((5, n, words, 16), dtype=torch.uint8, device="cuda:%d" % self.device)
        elif (tuple(buf.shape[:2]) != (5, n) or buf.shape[2] < words or tuple(buf.shape[3:]) != (16,)
              or buf.dtype != torch.uint8 or not buf.is_contiguous()):
            raise ValueError("buf must be a contiguous (5, n, >= words, 16) uint8 device tensor")
        buf = buf[:, :, :words]  # a padded slab: each field starts at its own row of the slab
        plain = torch.empty((words, 16), dtype=torch.uint8, device=buf.device) if with_plain else None
        ptrs = (C.c_void_p * (5 * n))(*[buf[k, j].data_ptr() for k in range(5) for j in range(n)])
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._check(lib.amph_synth_odos(self._h, seed, n, words, ptrs, _ptr(plain), fault_index,
                                        noncanon_permille, stream))
        odos = [tuple(buf[k, j] for k in range(5)) for j in range(n)]
        return odos, buf, plain

    def synth_words(self, seed: int, count: int, out=None):
        import torch
        if out is None:
            out = torch.empty((count, 16), dtype=torch.uint8, device="cuda:%d" % self.device)
        elif tuple(out.shape) != (count, 16) or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("out must be a contiguous (count, 16) uint8 device tensor")
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._check(lib.amph_synth_words(self._h, seed, count, _ptr(out), stream))
        return out


class PartySession:
    """One amph_party (include/amphora.h): a party's Output Delivery with the
    triples, diffs and ODO fields kept on the device between begin, the
    partners' texts and finish."""

    def __init__(self, ctx: Context, h, words: int, n_parties: int, yrv):
        self.ctx, self._h, self.words, self.n = ctx, h, words, n_parties
        self.y, self.r, self.v = yrv

    def text(self) -> bytes:
        """This party's interimValues text (the FactorPair JSON array)."""
        n = lib.amph_party_text_len(self._h)
        out = np.empty(max(n, 1), np.uint8)
        Context._check(lib.amph_party_text(self._h, _ptr(out), n))
        return out[:n].tobytes()

    def partner(self, slot: int, text):
        """A partner's interimValues text into slot 1..n-1; raises ValueError
        on a malformed text or a pair count other than 2 * words."""
        if isinstance(text, str):
            text = text.encode("utf-8")
        a = np.frombuffer(bytes(text), np.uint8)
        bad = C.c_int64(-1)
        st = lib.amph_party_partner(self._h, slot, _ptr(a) if a.size else None, a.size, C.byref(bad))
        if st in (AMPH_E_PARAM, AMPH_E_LEN) and bad.value >= 0:
            raise ValueError(lib.amph_last_error().decode())
        Context._check(st)

    def finish(self, is_player0: bool):
        """-> (w, u) as (W, 16) words."""
        w, u = np.empty((self.words, 16), np.uint8), np.empty((self.words, 16), np.uint8)
        Context._check(lib.amph_party_finish(self._h, int(is_player0), _ptr(w), _ptr(u)))
        return w, u

    def finish_b64(self, is_player0: bool):
        """-> the five ODO fields (secretShares, rShares, vShares, wShares,
        uShares) as base64 bytes."""
        nc = 4 * ((16 * self.words + 2) // 3)
        outs = [np.empty(max(nc, 1), np.uint8) for _ in range(5)]
        arr = (C.c_void_p * 5)(*[_ptr(o) for o in outs])
        Context._check(lib.amph_party_finish_b64(self._h, int(is_player0), arr))
        return [o[:nc].tobytes() for o in outs]

    def reset_partner(self, slot: int):
        """amph_party_reset_partner: free a slot whose text was rejected."""
        Context._check(lib.amph_party_reset_partner(self._h, slot))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.amph_party_free(self._h)
        self._h = None

    def __del__(self):
        if lib is not None:
            self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ClientSession:
    """One amph_client (include/amphora_client_session.h): each party's five
    base64 field texts are added into five running sums on the device as they
    arrive; the finish calls give what recombine_verify_b64 / mask_input_b64 /
    mask_input_json give on all the texts.  Host mode takes str / bytes /
    arrays, device mode (Context.client_begin_dev) uint8 device tensors and
    returns device tensors, asynchronous on the session's stream."""

    def __init__(self, ctx: Context, h, words: int, n_parties: int, stream):
        self.ctx, self._h, self.words, self.n, self.stream = ctx, h, words, n_parties, stream

    @property
    def dev(self) -> bool:
        return self.stream is not None

    def _sp(self):
        return C.c_void_p(self.stream.cuda_stream)

    def _verdict(self):
        if self.dev:
            import torch
            t = torch.empty(1, dtype=torch.int64, device="cuda:%d" % self.ctx.device)
            return t, C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_int64))
        v = C.c_int64(-1)
        return v, C.pointer(v)

    def _empty(self, shape):
        if self.dev:
            import torch
            return torch.empty(shape, dtype=torch.uint8, device="cuda:%d" % self.ctx.device)
        return np.empty(shape, np.uint8)

    @property
    def parties_seen(self) -> int:
        return int(lib.amph_client_parties_seen(self._h))

    def party(self, slot: int, five_texts, bad=None):
        """Party `slot`'s five field texts (ODO order) into the sums: one
        launch.  Host: returns -1, raises ValueError with the whole call's
        message on an illegal base64 character (the slot counts as taken).
        Device: returns the int64 (1,) verdict tensor (`bad`, or a new one)."""
        arr, keep = self.ctx._text_structs([five_texts])
        if self.dev:
            if not all(_is_dev(k) for k in keep):
                raise ValueError("a device-mode session takes device tensors")
            if bad is None:
                bad, _ = self._verdict()
            badp = C.cast(C.c_void_p(bad.data_ptr()), C.POINTER(C.c_int64))
            Context._check(lib.amph_client_party_dev(self._h, slot, arr, badp, self._sp()))
            return bad
        if any(_is_dev(k) for k in keep):
            raise ValueError("a host-mode session takes host buffers")
        v = C.c_int64(-1)
        st = lib.amph_client_party(self._h, slot, arr, C.byref(v))
        if st == AMPH_E_PARAM and v.value >= 0:
            raise ValueError(lib.amph_last_error().decode())
        Context._check(st)
        return v.value

    def _done(self, st, bad):
        if st == AMPH_E_PARAM and not self.dev and bad.value >= 0:
            raise ValueError(lib.amph_last_error().decode())
        if st == AMPH_E_PARAM and self.dev and lib.amph_last_error().startswith(b"Illegal base64 character"):
            raise ValueError(lib.amph_last_error().decode())
        Context._check(st, allow_verify=True)

    def finish_verify(self):
        """-> (canonical secrets (W, 16), first_fail, bad_char), as
        Context.recombine_verify_b64."""
        out = self._empty((self.words, 16))
        ff, ffp = self._verdict()
        bad, badp = self._verdict()
        if self.dev:
            st = lib.amph_client_finish_verify_dev(self._h, _ptr(out), ffp, badp, self._sp())
        else:
            st = lib.amph_client_finish_verify(self._h, _ptr(out), ffp, badp)
        self._done(st, bad)
        return out, Context._ff_value(ff), Context._ff_value(bad)

    def finish_mask(self, secrets16, records: bool = True, raw: bool = False):
        """-> (masked (S, 16) or None, records (S, 24) or None, first_fail,
        bad_char), as Context.mask_input_b64."""
        sv = words_view(secrets16)
        if _is_dev(sv) != self.dev:
            raise ValueError("secrets must live where the session's texts live")
        S = sv.shape[0]
        o16 = self._empty((S, 16)) if raw else None
        o24 = self._empty((S, 24)) if records else None
        ff, ffp = self._verdict()
        bad, badp = self._verdict()
        if self.dev:
            st = lib.amph_client_finish_mask_dev(self._h, _ptr(sv), S, _ptr(o16), _ptr(o24), ffp, badp, self._sp())
        else:
            st = lib.amph_client_finish_mask(self._h, _ptr(sv), S, _ptr(o16), _ptr(o24), ffp, badp)
        self._done(st, bad)
        return o16, o24, Context._ff_value(ff), Context._ff_value(bad)

    def finish_mask_json(self, secrets16):
        """-> (the MaskedInput "data" array text, first_fail, bad_char), as
        Context.mask_input_json."""
        sv = words_view(secrets16)
        if _is_dev(sv) != self.dev:
            raise ValueError("secrets must live where the session's texts live")
        S = sv.shape[0]
        cap = lib.amph_masked_input_data_chars(S)
        out = self._empty((cap,))
        ff, ffp = self._verdict()
        bad, badp = self._verdict()
        if self.dev:
            st = lib.amph_client_finish_mask_json_dev(self._h, _ptr(sv), S, _ptr(out), cap, ffp, badp, self._sp())
        else:
            st = lib.amph_client_finish_mask_json(self._h, _ptr(sv), S, _ptr(out), cap, ffp, badp)
        self._done(st, bad)
        return (out if self.dev else out.tobytes()), Context._ff_value(ff), Context._ff_value(bad)

    def word(self, i: int):
        """amph_client_word: the recombined (y, r, v, w, u) of word i as ints."""
        out = np.empty((5, 16), np.uint8)
        Context._check(lib.amph_client_word(self._h, i, _ptr(out)))
        return tuple(int.from_bytes(out[k].tobytes(), "little") for k in range(5))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.amph_client_free(self._h)
        self._h = None

    def __del__(self):
        if lib is not None:
            self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ClientSessions:
    """One amph_clients (include/amphora_client_batch.h): K secrets in one
    client session.  Each party's K responses arrive as five slotted field
    buffers (object o's text at field_offsets[o] of each, the layout
    PartySessions.finish_b64 writes) and are added into running sums in one
    launch; the finish calls give, per object, what the packed wire-text calls
    give on all parties' buffers.  Host mode takes uint8 arrays / bytes and
    returns numpy arrays with -1 for a clean verdict; device mode
    (Context.clients_begin_dev) takes and returns torch device tensors with
    AMPH_NO_FAILURE for a clean verdict, asynchronous on the session's stream."""

    def __init__(self, ctx: Context, h, word_offsets, n_parties: int, stream):
        self.ctx, self._h, self.n, self.stream = ctx, h, n_parties, stream
        self.word_offsets = word_offsets
        self.objects, self.words = int(word_offsets.size - 1), int(word_offsets[-1])
        self.field_chars = int(lib.amph_clients_field_chars(h))
        self.upload_chars = int(lib.amph_clients_upload_chars(h))
        self.field_offsets = np.empty(self.objects, np.uint64)
        self.upload_offsets = np.empty(self.objects, np.uint64)
        Context._check(lib.amph_clients_field_offsets(h, _ptr(self.field_offsets)))
        Context._check(lib.amph_clients_upload_offsets(h, _ptr(self.upload_offsets)))

    @property
    def dev(self) -> bool:
        return self.stream is not None

    def _sp(self):
        return C.c_void_p(self.stream.cuda_stream)

    def _array(self, shape, dtype="uint8"):
        if self.dev:
            import torch
            return torch.empty(shape, dtype=getattr(torch, dtype), device="cuda:%d" % self.ctx.device)
        return np.empty(shape, dtype=dtype)

    @property
    def parties_seen(self) -> int:
        return int(lib.amph_clients_parties_seen(self._h))

    def object_words(self, o: int) -> int:
        return int(self.word_offsets[o + 1] - self.word_offsets[o])

    def field_lens(self):
        return [wire_text_chars(self.object_words(o)) for o in range(self.objects)]

    def pack_texts(self, texts_by_object):
        """K x 5 strings (texts_by_object[o][k]: object o's field k, ODO order)
        -> the five slotted buffers (uint8 arrays of field_chars characters;
        what lies between the texts is 0).  A text of another length than its
        object's raises AmphoraNativeError(AMPH_E_LEN)."""
        _need(len(texts_by_object) == self.objects,
              "expected %d objects' texts, got %d" % (self.objects, len(texts_by_object)))
        bufs = np.zeros((5, max(self.field_chars, 1)), np.uint8)
        for o, (five, nc) in enumerate(zip(texts_by_object, self.field_lens())):
            _need(len(five) == 5, "object %d: five base64 fields" % o)
            at = int(self.field_offsets[o])
            for k, t in enumerate(five):
                if isinstance(t, str):
                    t = t.encode("ascii", errors="replace")
                a = np.frombuffer(bytes(t), np.uint8)
                if a.size != nc:
                    raise AmphoraNativeError(AMPH_E_LEN, "object %d: base64 fields of %d characters, expected %d "
                                                         "for %d words" % (o, a.size, nc, self.object_words(o)))
                bufs[k, at:at + nc] = a
        return [bufs[k, :self.field_chars] for k in range(5)]

    def party(self, slot: int, five_buffers, bad=None, status: bool = False):
        """Party `slot`'s five slotted field buffers (ODO order) into the sums:
        one launch whatever K is.  Host: -> this call's bad_chars[K] (-1
        clean); raises ValueError with the packed calls' message when any
        object holds an illegal character, unless status (then -> (bad_chars,
        (status, message))); the slot counts as taken either way.  Device:
        the buffers of a PartySessionsDev.finish_b64 go in unchanged; -> the
        int64 (K,) verdict tensor (`bad`, or a new one)."""
        if self.dev and any(b is None for b in five_buffers):  # (a session of empty objects only)
            five_buffers = [self._array((0,)) for _ in range(5)]
        arr, keep = self.ctx._text_structs([five_buffers])
        if self.dev:
            if not all(_is_dev(k) for k in keep):
                raise ValueError("a device-mode session takes device tensors")
            if bad is None:
                bad = self._array((self.objects,), "int64")
            Context._check(lib.amph_clients_party_dev(self._h, slot, arr, _ptr(bad), self._sp()))
            return bad
        if any(_is_dev(k) for k in keep):
            raise ValueError("a host-mode session takes host buffers")
        v = np.full(self.objects, -1, np.int64)
        st = lib.amph_clients_party(self._h, slot, arr, _ptr(v))
        msg = lib.amph_last_error().decode() if st != AMPH_OK else ""
        if st == AMPH_E_PARAM and (v >= 0).any():
            if status:
                return v, (st, msg)
            raise ValueError(msg)
        Context._check(st)
        return (v, (st, msg)) if status else v

    def party_texts(self, slot: int, texts_by_object, status: bool = False):
        """party() on K x 5 host strings, gathered into the slotted buffers."""
        bufs = self.pack_texts(texts_by_object)
        if self.dev:
            import torch
            with torch.cuda.stream(self.stream):  # the upload is ordered before the launch that reads it
                bufs = [torch.from_numpy(np.ascontiguousarray(b)).to("cuda:%d" % self.ctx.device) for b in bufs]
            return self.party(slot, bufs)
        return self.party(slot, bufs, status=status)

    def scan_bodies(self, bodies):
        """K bodies (bytes) -> the (K, 5) uint64 starts for party_bodies, by
        bodies_scan; a member of another length than its object's raises
        AmphoraNativeError(AMPH_E_LEN), a body that is not plain BodyNotPlain."""
        _need(len(bodies) == self.objects, "expected %d bodies, got %d" % (self.objects, len(bodies)))
        starts = np.empty((self.objects, 5), np.uint64)
        for o, (b, nc) in enumerate(zip(bodies, self.field_lens())):
            starts[o], lens = bodies_scan(b)
            if (lens != nc).any():
                raise AmphoraNativeError(AMPH_E_LEN, "object %d: base64 fields of %s characters, expected %d for %d "
                                                     "words" % (o, [int(x) for x in lens], nc, self.object_words(o)))
        return starts

    def party_bodies(self, slot: int, bodies, starts=None, status: bool = False):
        """amph_bodies_party: party `slot`'s K response bodies (bytes) as they
        are -- K pointers to the K objects, no join, no gather; starts: the
        (K, 5) byte starts of the five members inside each body (scan_bodies
        when None), AMPH_BODY_ABSENT in a row marks the object absent.  One
        launch whatever K is.  Raises ValueError with the packed calls'
        message when any object holds an illegal character, unless status
        (then -> (status, message)); the slot counts as taken either way.  A
        device-mode session lays the bodies out in one device buffer
        (party_bodies_dev takes a buffer that is already there)."""
        if starts is None:
            starts = self.scan_bodies(bodies)
        st_ = np.ascontiguousarray(starts, dtype=np.uint64)
        _need(st_.shape == (self.objects, 5) and len(bodies) == self.objects,
              "one body and five starts per object (%d objects)" % self.objects)
        if self.dev:
            import torch
            at = np.concatenate([[0], np.cumsum([(len(b) + 15) & ~15 for b in bodies])]).astype(np.uint64)
            buf = np.zeros(max(int(at[-1]), 16), np.uint8)
            for b, a in zip(bodies, at):
                buf[int(a):int(a) + len(b)] = np.frombuffer(bytes(b), np.uint8)
            with torch.cuda.stream(self.stream):  # the upload is ordered before the launch that reads it
                dbuf = torch.from_numpy(buf).to("cuda:%d" % self.ctx.device)
            absent = (st_ == AMPH_BODY_ABSENT).any(axis=1)
            return self.party_bodies_dev(slot, dbuf, np.where(absent[:, None], st_, st_ + at[:-1, None]))
        K = self.objects
        ptrs = (C.c_char_p * K)(*[bytes(b) if not isinstance(b, bytes) else b for b in bodies])
        lens = (C.c_size_t * K)(*[len(b) for b in bodies])
        st = lib.amph_bodies_party(self._h, slot, ptrs, lens, _ptr(st_))
        msg = lib.amph_last_error().decode() if st != AMPH_OK else ""
        if st == AMPH_E_PARAM and msg.startswith("object ") and "Illegal base64 character" in msg:
            if status:
                return st, msg
            raise ValueError(msg)
        Context._check(st)
        return (st, msg) if status else None

    def party_bodies_dev(self, slot: int, buffer, starts):
        """amph_bodies_party_dev: `buffer` is a uint8 device tensor (16-byte
        aligned) that holds the K bodies anywhere, starts the (K, 5) absolute
        byte starts (a host array).  Only enqueues; the buffer must stay alive
        until the session's stream has run the launch."""
        st_ = np.ascontiguousarray(starts, dtype=np.uint64)
        _need(st_.shape == (self.objects, 5), "five starts per object (%d objects)" % self.objects)
        if not self.dev or not _is_dev(buffer):
            raise ValueError("a device-mode session and a device tensor")
        Context._check(lib.amph_bodies_party_dev(self._h, slot, _ptr(buffer), buffer.numel(), _ptr(st_), self._sp()))

    def _verdicts(self):
        """(first_fails, bad_chars): host arrays start at -1, so a call that is
        refused before it writes them reports no verdict."""
        if self.dev:
            return self._array((self.objects,), "int64"), self._array((self.objects,), "int64")
        return np.full(self.objects, -1, np.int64), np.full(self.objects, -1, np.int64)

    def _done(self, st, res, bad, status):
        """Per-object verdicts are the result: AMPH_E_VERIFY, and AMPH_E_PARAM
        with a bad character reported in bad_chars, return them (status=True
        appends (status, amph_last_error)); anything else raises."""
        msg = lib.amph_last_error().decode() if st != AMPH_OK else ""
        if not (st == AMPH_E_PARAM and not self.dev and (bad >= 0).any()):
            Context._check(st, allow_verify=True)
        return res + ((st, msg),) if status else res

    def finish_verify(self, status: bool = False):
        """-> (canonical secrets (T, 16) packed on word_offsets, first_fails[K],
        bad_chars[K]), as Context.recombine_verify_b64_packed."""
        out = self._array((self.words, 16))
        ff, bad = self._verdicts()
        if self.dev:
            st = lib.amph_clients_finish_verify_dev(self._h, _ptr(out), _ptr(ff), _ptr(bad), self._sp())
        else:
            st = lib.amph_clients_finish_verify(self._h, _ptr(out), _ptr(ff), _ptr(bad))
        return self._done(st, (out, ff, bad), bad, status)

    def _secrets(self, secrets16):
        sv = words_view(secrets16)
        if _is_dev(sv) != self.dev:
            raise ValueError("secrets must live where the session's texts live")
        _need(sv.shape[0] == self.words, "one secret per input mask word: expected %d, got %d" % (
            self.words, sv.shape[0]))
        return sv

    def finish_mask(self, secrets16, records: bool = True, raw: bool = False, status: bool = False):
        """-> (masked (T, 16) or None, records (T, 24) or None, first_fails[K],
        bad_chars[K]), as Context.mask_input_b64_packed."""
        sv = self._secrets(secrets16)
        o16 = self._array((self.words, 16)) if raw else None
        o24 = self._array((self.words, 24)) if records else None
        ff, bad = self._verdicts()
        if self.dev:
            st = lib.amph_clients_finish_mask_dev(self._h, _ptr(sv), _ptr(o16), _ptr(o24), _ptr(ff), _ptr(bad),
                                                  self._sp())
        else:
            st = lib.amph_clients_finish_mask(self._h, _ptr(sv), _ptr(o16), _ptr(o24), _ptr(ff), _ptr(bad))
        return self._done(st, (o16, o24, ff, bad), bad, status)

    def finish_mask_json(self, secrets16, out=None, status: bool = False):
        """-> (the framed texts: one uint8 buffer of upload_chars characters
        with object o's "data" array text at upload_offsets[o], first_fails[K],
        bad_chars[K]), as Context.mask_input_json_packed; the buffer goes into
        Context.convert_share_json_packed unchanged.  `out`: write into the
        caller's buffer (what lies between the texts stays as it is)."""
        sv = self._secrets(secrets16)
        if out is None:
            out = self._array((max(self.upload_chars, 1),))
            out[:] = 0
        cap = int(out.numel() if self.dev else out.size)
        ff, bad = self._verdicts()
        if self.dev:
            st = lib.amph_clients_finish_mask_json_dev(self._h, _ptr(sv), _ptr(out), cap, _ptr(ff), _ptr(bad),
                                                       self._sp())
        else:
            st = lib.amph_clients_finish_mask_json(self._h, _ptr(sv), _ptr(out), cap, _ptr(ff), _ptr(bad))
        return self._done(st, (out, ff, bad), bad, status)

    def split_upload(self, text):
        """finish_mask_json's buffer (host) -> the K framed texts (bytes)."""
        return [bytes(text[int(a):int(a) + masked_input_data_chars(self.object_words(o))])
                for o, a in enumerate(self.upload_offsets)]

    def word(self, o: int, i: int):
        """amph_clients_word: the recombined (y, r, v, w, u) of word i of object o as ints."""
        out = np.empty((5, 16), np.uint8)
        Context._check(lib.amph_clients_word(self._h, o, i, _ptr(out)))
        return tuple(int.from_bytes(out[k].tobytes(), "little") for k in range(5))

    def close(self):
        # (a session finalised after its context -- the collector's order in a
        # reference cycle is arbitrary -- must not touch the destroyed context)
        if getattr(self, "_h", None) is not None and self._h.value and getattr(self.ctx, "_h", None) is not None:
            lib.amph_clients_free(self._h)
        self._h = None

    def __del__(self):
        if lib is not None:
            self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _DevArray:  # a device address as __cuda_array_interface__ (torch.as_tensor views it)
    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _dev_view(ptr: int, n: int, typestr: str, device: int):
    import torch
    return torch.as_tensor(_DevArray(ptr, n, typestr), device="cuda:%d" % device)


class PartySessionDev(PartySession):
    """A device-mode amph_party (amph_party_*_dev): torch device tensors in
    and out, every call asynchronous on torch's current stream."""

    def __init__(self, ctx: Context, h, words: int, n_parties: int, yrv, keep):
        super().__init__(ctx, h, words, n_parties, yrv)
        self._keep = keep  # the tuples, read in place until finish

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.ctx.device).cuda_stream)

    def text_dev(self):
        """-> (this party's text: a uint8 device tensor of the text's capacity,
        its length: an int64 (1,) device tensor), both views of session memory
        (amph_party_text_dev), valid once the stream has run begin."""
        t, n = C.c_void_p(), C.c_void_p()
        Context._check(lib.amph_party_text_dev(self._h, C.byref(t), C.byref(n)))
        cap = lib.amph_exchange_max_chars(2 * self.words)
        return _dev_view(t.value, cap, "|u1", self.ctx.device), _dev_view(n.value, 1, "<i8", self.ctx.device)

    def text(self) -> bytes:
        """Synchronises and copies this party's text to the host (tests)."""
        t, n = self.text_dev()
        L = int(n.item())
        return t[:L].cpu().numpy().tobytes()

    def partner(self, slot: int, text, bad=None):
        """A partner's text (a uint8 device tensor) into slot 1..n-1; bad: an
        int64 (1,) device tensor the decode reports into (returned)."""
        import torch
        if bad is None:
            bad = torch.empty(1, dtype=torch.int64, device=text.device)
        Context._check(lib.amph_party_partner_dev(self._h, slot, _ptr(text) if text.numel() else None,
                                                  text.numel(), _ptr(bad), self._stream()))
        return bad

    def finish(self, is_player0: bool):
        raise AmphoraNativeError(AMPH_E_PARAM, "a device-mode session finishes with finish_b64")

    def finish_b64(self, is_player0: bool):
        """-> the five fields' base64 text: uint8 device tensors viewing the
        session's memory (valid until close)."""
        nc = 4 * ((16 * self.words + 2) // 3)
        arr = (C.c_void_p * 5)()
        Context._check(lib.amph_party_finish_b64_dev(self._h, int(is_player0), arr, self._stream()))
        return [_dev_view(arr[k], nc, "|u1", self.ctx.device) if nc else None for k in range(5)]



class PartySessions:
    """One amph_parties (include/amphora_party_batch.h): K Output Delivery
    requests of one party, device-resident from the packed tuples to the K
    responses' base64 fields.  Object o's interimValues text lies at
    text_offsets[o] of one buffer of text_bytes characters (every party of the
    exchange has the same layout), its field texts at field_offsets[o] of five
    buffers of field_chars characters."""

    def __init__(self, ctx: Context, h, word_offsets, n_parties: int, yrv):
        self.ctx, self._h, self.n = ctx, h, n_parties
        self.word_offsets = word_offsets
        self.objects, self.words = int(word_offsets.size - 1), int(word_offsets[-1])
        self.y, self.r, self.v = yrv
        self.text_bytes = int(lib.amph_parties_text_bytes(h))
        self.field_chars = int(lib.amph_parties_field_chars(h))
        self.text_offsets = np.empty(self.objects, np.uint64)
        self.field_offsets = np.empty(self.objects, np.uint64)
        Context._check(lib.amph_parties_text_offsets(h, _ptr(self.text_offsets)))
        Context._check(lib.amph_parties_field_offsets(h, _ptr(self.field_offsets)))

    def field_lens(self):
        return [wire_text_chars(int(self.word_offsets[o + 1] - self.word_offsets[o])) for o in range(self.objects)]

    def text_lens(self):
        out = np.empty(self.objects, np.uint64)
        Context._check(lib.amph_parties_text_lens(self._h, _ptr(out)))
        return out

    def text_buffer(self):
        """-> (the whole text buffer as a uint8 array, the K text lengths)."""
        out = np.empty(max(self.text_bytes, 1), np.uint8)
        Context._check(lib.amph_parties_text(self._h, AMPH_PARTIES_ALL, _ptr(out), self.text_bytes))
        return out[:self.text_bytes], self.text_lens()

    def text(self, o: int) -> bytes:
        """Object o's interimValues text (the FactorPair JSON array)."""
        n = int(self.text_lens()[o])
        out = np.empty(max(n, 1), np.uint8)
        Context._check(lib.amph_parties_text(self._h, o, _ptr(out), n))
        return out[:n].tobytes()

    def texts(self):
        buf, lens = self.text_buffer()
        return [buf[int(a):int(a) + int(n)].tobytes() for a, n in zip(self.text_offsets, lens)]

    def pack_texts(self, texts):
        """K texts (bytes) -> (one buffer at the session's offsets, their lengths)."""
        _need(len(texts) == self.objects, "expected %d texts, got %d" % (self.objects, len(texts)))
        buf, lens = np.zeros(max(self.text_bytes, 1), np.uint8), np.zeros(self.objects, np.uint64)
        for o, t in enumerate(texts):
            if isinstance(t, str):
                t = t.encode("utf-8")
            at = int(self.text_offsets[o])
            room = (int(self.text_offsets[o + 1]) if o + 1 < self.objects else self.text_bytes) - at
            lens[o] = len(t)
            if len(t) <= room:  # (a longer one is refused by the call, by its length)
                buf[at:at + len(t)] = np.frombuffer(bytes(t), np.uint8)
        return buf[:self.text_bytes], lens

    def partner(self, slot: int, texts, text_lens=None, status: bool = False):
        """One partner's K texts into slot 1..n-1: a list of K texts, or one
        buffer at the session's offsets with its lengths.  -> the K verdicts
        (int64: -1 clean, else the offending offset / the length on a count
        mismatch); raises ValueError when any text was refused unless status
        (then -> (verdicts, status))."""
        if text_lens is None:
            texts, text_lens = self.pack_texts(texts)
        buf = np.ascontiguousarray(texts, dtype=np.uint8)
        lens = np.ascontiguousarray(text_lens, dtype=np.uint64)
        _need(lens.size == self.objects, "one text length per object")
        _need(buf.size >= self.text_bytes, "the text buffer holds %d characters" % self.text_bytes)
        bad = np.full(self.objects, -1, np.int64)
        st = lib.amph_parties_partner(self._h, slot, _ptr(buf) if buf.size else None, _ptr(lens), _ptr(bad))
        if st in (AMPH_E_PARAM, AMPH_E_LEN) and (bad >= 0).any():
            if status:
                return bad, st
            raise ValueError(lib.amph_last_error().decode())
        Context._check(st)
        return (bad, st) if status else bad

    def reset_partner(self, slot: int):
        Context._check(lib.amph_parties_reset_partner(self._h, slot))

    def finish(self, is_player0: bool):
        """-> the packed (w, u) as (T, 16) words."""
        w, u = np.empty((self.words, 16), np.uint8), np.empty((self.words, 16), np.uint8)
        Context._check(lib.amph_parties_finish(self._h, int(is_player0), _ptr(w), _ptr(u)))
        return w, u

    def finish_b64(self, is_player0: bool):
        """-> (the five slotted field buffers as uint8 arrays of field_chars
        characters, rejected: K bytes 0 / 1)."""
        outs = [np.empty(max(self.field_chars, 1), np.uint8) for _ in range(5)]
        rej = np.zeros(self.objects, np.uint8)
        arr = (C.c_void_p * 5)(*[_ptr(o) for o in outs])
        Context._check(lib.amph_parties_finish_b64(self._h, int(is_player0), arr, _ptr(rej)))
        return [o[:self.field_chars] for o in outs], rej

    def split_fields(self, fields):
        """The slotted buffers of finish_b64 -> per object the five texts (bytes)."""
        fl = self.field_lens()
        return [[bytes(f[int(a):int(a) + n]) for f in fields] for a, n in zip(self.field_offsets, fl)]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.amph_parties_free(self._h)
        self._h = None

    def __del__(self):
        if lib is not None:
            self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class PartySessionsDev(PartySessions):
    """A device-mode amph_parties (amph_parties_*_dev): torch device tensors
    in and out, every call asynchronous on torch's current stream; close() is
    the one call that waits."""

    def __init__(self, ctx: Context, h, word_offsets, n_parties: int, yrv, keep):
        super().__init__(ctx, h, word_offsets, n_parties, yrv)
        self._keep = keep  # the tuples, read in place until finish

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.ctx.device).cuda_stream)

    def text_dev(self):
        """-> (the text buffer: uint8 (text_bytes,), its offsets: int64 (K,),
        the lengths: int64 (K,)), device tensors viewing session memory."""
        t, o, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        Context._check(lib.amph_parties_text_dev(self._h, C.byref(t), C.byref(o), C.byref(n)))
        d = self.ctx.device
        return (_dev_view(t.value, self.text_bytes, "|u1", d), _dev_view(o.value, self.objects, "<i8", d),
                _dev_view(n.value, self.objects, "<i8", d))

    def text_lens(self):
        return self.text_dev()[2].cpu().numpy().astype(np.uint64)

    def text_buffer(self):
        """Synchronises and copies the buffer and the lengths to the host (tests)."""
        t, _, n = self.text_dev()
        return t.cpu().numpy(), n.cpu().numpy().astype(np.uint64)

    def text(self, o: int) -> bytes:
        return self.texts()[o]

    def partner(self, slot: int, texts, text_lens, bad=None):
        """A partner's text buffer and lengths (device tensors, e.g. its
        text_dev()) into slot 1..n-1; bad: an int64 (K,) device tensor the
        decode reports into (returned)."""
        import torch
        if bad is None:
            bad = torch.empty(self.objects, dtype=torch.int64, device=texts.device)
        Context._check(lib.amph_parties_partner_dev(self._h, slot, _ptr(texts), _ptr(text_lens), _ptr(bad),
                                                    self._stream()))
        return bad

    def finish(self, is_player0: bool):
        raise AmphoraNativeError(AMPH_E_PARAM, "a device-mode session finishes with finish_b64")

    def finish_b64(self, is_player0: bool):
        """-> the five slotted field buffers: uint8 device tensors viewing the
        session's memory (valid until close)."""
        arr = (C.c_void_p * 5)()
        Context._check(lib.amph_parties_finish_b64_dev(self._h, int(is_player0), arr, self._stream()))
        return [_dev_view(arr[k], self.field_chars, "|u1", self.ctx.device) if self.field_chars else None
                for k in range(5)]
