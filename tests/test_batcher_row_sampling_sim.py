"""mmi_batcher_open_with on the simulator, and the server's query string (CPU only, stub batcher)."""
import asyncio

import pytest

from moshi_amd import SessionSampling
from moshi_amd import server as srv
from tests import row_sampling_cases as rc


def test_batcher_channels_with_their_own_settings(sim_lib):
    rc.check_batcher_channels("cpu", sim_lib)


def test_query_string_maps_to_session_sampling():
    q = {"text_temperature": "0.5", "text_topk": "12", "audio_temperature": "0.9", "audio_topk": "100", "pad_mult": "-1.5",
         "repetition_penalty": "1.25", "repetition_penalty_context": "32", "text_seed": "42", "audio_seed": "7", "other": "x"}
    s = srv.parse_session_query(q)
    assert s == SessionSampling(temp=0.9, temp_text=0.5, top_k=100, top_k_text=12, seed=42, pad_mult=-1.5, repetition_penalty=1.25,
                                repetition_context=32)
    assert srv.parse_session_query({"seed": "9", "text_seed": "1"}).seed == 9          # text_seed is only a synonym
    assert srv.parse_session_query({}) is None and srv.parse_session_query(None) is None
    assert srv.parse_session_query({"audio_seed": "3", "worker_auth_id": "k"}) is None   # nothing the engine takes


@pytest.mark.parametrize("q,exc", [({"text_topk": "300"}, NotImplementedError), ({"audio_topk": "-1"}, ValueError),
                                   ({"repetition_penalty": "0"}, ValueError), ({"repetition_penalty_context": "65"}, ValueError),
                                   ({"pad_mult": "nan"}, ValueError), ({"text_temperature": "inf"}, ValueError),
                                   ({"text_topk": "many"}, ValueError), ({"seed": "-1"}, ValueError)])
def test_query_values_the_engine_would_refuse_are_refused(q, exc):
    with pytest.raises(exc):
        srv.parse_session_query(q)


class _Ws:
    def __init__(self):
        self.sent, self.closed = [], False

    async def send_bytes(self, b):
        self.sent.append(b)

    async def close(self):
        self.closed = True

    def __aiter__(self):
        return self

    async def __anext__(self):
        raise StopAsyncIteration


class _Batcher:
    frame_size = 4

    def __init__(self):
        self.opened = []

    def open(self, *args, **kw):
        self.opened.append((args, kw))
        return len(self.opened)

    def close(self, ch):
        pass


def test_a_refused_query_closes_the_connection_before_a_slot_is_claimed():
    b = _Batcher()
    server = srv.BatchedServer(b)
    ws = _Ws()
    asyncio.run(server.serve_websocket(ws, {"text_topk": "1000"}))
    assert ws.closed and not b.opened
    kind, text = srv.decode_message(ws.sent[0])
    assert kind == srv.MT_ERROR and "top_k" in text


def test_query_settings_reach_open_and_no_query_opens_as_before():
    b = _Batcher()
    server = srv.BatchedServer(b)
    asyncio.run(server.serve_websocket(_Ws(), {"seed": "5", "pad_mult": "0.5"}))
    asyncio.run(server.serve_websocket(_Ws()))
    asyncio.run(server.serve_websocket(_Ws(), {}))
    assert b.opened[0] == ((), {"sampling": SessionSampling(seed=5, pad_mult=0.5)})
    assert b.opened[1] == ((), {}) and b.opened[2] == ((), {})
