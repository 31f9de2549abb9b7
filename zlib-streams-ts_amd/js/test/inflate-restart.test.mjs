// Restart points through the JavaScript host path (streams-api.mjs -> zsnapi.node ->
// zs_pool_inflate_batch_restart): decompressBatch*(inputs, format, {outCapacity, restartPoints}) on
// streams that node's own zlib flushed, and the rejection rules.
//   node inflate-restart.test.mjs cpu   -- the argument checks only (no GPU needed)
import zlib from "zlib";

import * as corpus from "../../../tests/golden/corpus.mjs";
import * as api from "../streams-api.mjs";

let checks = 0;
const expect = (c, m) => { if (!c) throw new Error("FAIL " + m); checks++; };
const same = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.length), Buffer.from(b.buffer, b.byteOffset, b.length)) === 0;

async function rejects(p, pred, what) {
  let e = null;
  try { await p; } catch (x) { e = x; }
  expect(e !== null && pred(e), what + (e ? ": " + e.message : ": no error"));
}

async function argumentChecks() {
  const one = [new Uint8Array([1, 2, 3, 4, 5, 6, 7, 8])];
  const type = (e) => e instanceof TypeError;
  const ok = { outCapacity: 64, restartPoints: [[[7, 1]]] };
  await rejects(api.decompressBatch(one, "deflate", { restartPoints: [[[7, 1]]] }), type, "without outCapacity: a TypeError");
  await rejects(api.decompressBatch(one, "deflate", { ...ok, dictionary: new Uint8Array(4) }), type, "with a dictionary: a TypeError");
  await rejects(api.decompressBatchSettled(one, "deflate64-raw", ok), type, "deflate64-raw: a TypeError");
  for (const restartPoints of [3, [], [[], []], [7], [[7, 1]], [[[7]]], [[[7, 1, 2]]], [[[1.5, 1]]], [[[7, -1]]], [[["7", 1]]],
                               [[[2 ** 32, 1]]]])
    await rejects(api.decompressBatchDetailed(one, "deflate", { outCapacity: 64, restartPoints }), type,
                  JSON.stringify(restartPoints) + ": a TypeError");
  // the wrapper's header
  const gz = (flg, rest) => new Uint8Array([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 3, ...rest]);
  expect(api.wrapperHeaderLength(one[0], "deflate-raw") === 0 && api.wrapperHeaderLength(one[0], "deflate") === 2, "raw 0, zlib 2");
  expect(api.wrapperHeaderLength(gz(0, [3, 0])) === 10, "a plain gzip header");
  expect(api.wrapperHeaderLength(gz(8, [97, 0, 3, 0])) === 12, "FNAME");
  expect(api.wrapperHeaderLength(gz(4 | 16 | 2, [2, 0, 9, 9, 99, 0, 1, 2, 3])) === 18, "FEXTRA, FCOMMENT, FHCRC");
  expect(api.wrapperHeaderLength(gz(8, [97, 98])) === 0 && api.wrapperHeaderLength(gz(0x20, [])) === 0, "truncated, reserved flag");
  expect(api.wrapperHeaderLength(zlib.gzipSync(Buffer.from("x"))) === 10, "node's gzip header");
}

// x compressed by node's zlib with a full flush at every position of `at`: [stream, [[inPos, outPos]]]
function flushed(x, at, format) {
  const mk = { "deflate-raw": zlib.createDeflateRaw, deflate: zlib.createDeflate, gzip: zlib.createGzip }[format];
  return new Promise((resolve, reject) => {
    const z = mk({ level: 6 });
    const chunks = [], points = [];
    let total = 0;
    z.on("data", (c) => { chunks.push(c); total += c.length; });
    z.on("error", reject);
    z.on("end", () => resolve([new Uint8Array(Buffer.concat(chunks)), points]));
    const step = (k, from) => {
      if (k === at.length) return z.end(Buffer.from(x.subarray(from)));
      z.write(Buffer.from(x.subarray(from, at[k])));
      z.flush(zlib.constants.Z_FULL_FLUSH, () => { points.push([total, at[k]]); step(k + 1, at[k]); });
    };
    step(0, 0);
  });
}

async function main() {
  await argumentChecks();
  if (process.argv[2] === "cpu") {
    console.log("ok " + checks);
    return;
  }
  const x = corpus.text(corpus.streamSeed(77), 150000);
  for (const format of ["deflate-raw", "deflate", "gzip"]) {
    const made = [await flushed(x, [65536, 70001], format), await flushed(x.subarray(0, 100), [4, 8], format),
                  await flushed(x.subarray(0, 3), [0, 1, 3], format)];
    const srcs = [x, x.subarray(0, 100), x.subarray(0, 3)];
    const ins = made.map((m) => m[0]);
    const options = { outCapacity: [150000, 100, 3], restartPoints: made.map((m) => m[1]) };
    const outs = await api.decompressBatch(ins, format, options);
    outs.forEach((o, i) => expect(same(o, srcs[i]), `${format}: input ${i} from its restart points`));
    const d = await api.decompressBatchDetailed(ins, format, options);
    expect(d.consumed[0] === ins[0].length && d.status[0] === 1, format + ": the whole stream is consumed");
    // a wrong point fails that stream alone, by status and message
    const bad = { ...options, restartPoints: [made[0][1], [[made[1][1][0][0] + 1, 4]], null] };
    const s = await api.decompressBatchSettled(ins, format, bad);
    expect(s[0].status === "fulfilled" && same(s[0].value, x), format + ": the neighbour of a broken stream");
    expect(s[1].status === "rejected" && s[1].reason.message === "process error: -3" &&
           s[1].reason.zmsg === "restart points do not decode the stream", format + ": the one failure");
    expect(s[2].status === "fulfilled" && same(s[2].value, srcs[2]), format + ": null is the plain stream");
    // points the entry refuses
    await rejects(api.decompressBatch(ins, format, { ...options, restartPoints: [[[9, 5], [10, 6]], null, null] }),
                  (e) => e.message === "init failed: -2" && e.code === "-2", format + ": points out of order");
  }
  console.log("ok " + checks);
}

main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
