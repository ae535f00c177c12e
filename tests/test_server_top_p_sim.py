"""The websocket server with `text_topp` / `audio_topp` in the connection URL, on the CPU kernel simulator: a batcher
with the nucleus samplers serves the connection with its own top_p, one without them answers with the protocol's Error message."""
import asyncio

import numpy as np

from moshi_amd import server as srv
from tests import batcher_cases
from tests.test_server import _client

QUERY = {"text_topp": "0.9", "audio_topp": "0.8", "seed": "4711", "text_temperature": "0.7"}


def _serve(batcher, url_query, inputs, n_expect):
    import aiohttp
    from aiohttp import web

    async def scenario():
        server = srv.BatchedServer(batcher, model_version=3)
        server.start()
        runner = web.AppRunner(server.make_app())
        await runner.setup()
        site = web.TCPSite(runner, "127.0.0.1", 0)
        await site.start()
        port = site._server.sockets[0].getsockname()[1]
        try:
            async with aiohttp.ClientSession() as session:
                return await _client(session, f"http://127.0.0.1:{port}/api/chat?{url_query}", inputs, 4096, n_expect), list(server.errors)
        finally:
            server.stop()
            await runner.cleanup()
    return asyncio.run(scenario())


def test_a_connection_with_text_topp_is_served_with_its_own_nucleus(sim_lib):
    from moshi_amd.batcher import SessionBatcher
    slots, n_frames = 2, 5
    mimi, lm, mcfg, lcfg = batcher_cases.tiny_pair("cpu", sim_lib, slots)
    rng = np.random.default_rng(3)
    inputs = [(0.3 * rng.standard_normal(mcfg.frame_size)).astype(np.float32) for _ in range(n_frames)]
    url_query = "&".join(f"{k}={v}" for k, v in QUERY.items())

    def alone(sampling):
        with SessionBatcher(mimi, lm, slots, use_sampling=True, seed=11, session_top_p=True) as b:
            ch = b.open(sampling=sampling)
            b.push(ch, np.concatenate(inputs))
            outs = []
            while b.step() > 0:
                while (fr := b.pop(ch)) is not None:
                    outs.append(fr)
            return outs
    want = alone(srv.parse_session_query(QUERY))
    without = alone(srv.parse_session_query({k: v for k, v in QUERY.items() if "topp" not in k}))
    assert 0 < len(want) < n_frames
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(want, without)), "the nucleus changed no token: nothing shown"

    with SessionBatcher(mimi, lm, slots, use_sampling=True, seed=11, session_top_p=True) as batcher:
        (hello, pcm, text), errors = _serve(batcher, url_query, inputs, len(want))
    assert not errors, errors
    assert hello == (srv.MT_HANDSHAKE, (0, 3))
    assert len(pcm) == len(want)
    for f in range(len(want)):
        assert np.array_equal(pcm[f], want[f][0]), f"frame {f}: audio differs from the batcher's own output with the same settings"
    assert text == [str(int(tok[0])) for _, tok in want if int(tok[0]) not in (0, 3)]


def test_a_batcher_without_the_nucleus_samplers_answers_text_topp_with_an_error_message(sim_lib):
    from moshi_amd.batcher import SessionBatcher
    slots = 2
    mimi, lm, mcfg, lcfg = batcher_cases.tiny_pair("cpu", sim_lib, slots)
    inputs = [np.zeros(mcfg.frame_size, np.float32)]
    with SessionBatcher(mimi, lm, slots, use_sampling=True, seed=11) as batcher:
        (hello, pcm, text), errors = _serve(batcher, "text_topp=0.9", inputs, 0)
        assert hello[0] == srv.MT_ERROR and "bad sampling parameters" in hello[1] and "nucleus" in hello[1], hello
        assert batcher.used_slots == 0 and not errors
        (hello, pcm, text), errors = _serve(batcher, "audio_topp=1.5", inputs, 0)          # out of the domain: the parser's refusal
        assert hello[0] == srv.MT_ERROR and "bad sampling parameters" in hello[1]
        (hello, pcm, text), errors = _serve(batcher, "text_topp=0", inputs, 0)             # off: served as before
        assert hello == (srv.MT_HANDSHAKE, (0, 3)) and not errors
