// Restart points found by the engine, through the JavaScript host path (streams-api.mjs -> zsnapi.node ->
// zs_pool_inflate_batch_sync): decompressBatch*(inputs, format, {outCapacity, restartPoints: "scan"}) on
// streams that node's own zlib flushed, and the rejection rules.
//   node inflate-sync.test.mjs cpu   -- the argument checks only (no GPU needed)
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
  await rejects(api.decompressBatch(one, "deflate", { restartPoints: "scan" }), type, "without outCapacity: a TypeError");
  await rejects(api.decompressBatch(one, "deflate", { outCapacity: 64, restartPoints: "scan", dictionary: new Uint8Array(4) }), type,
                "with a dictionary: a TypeError");
  await rejects(api.decompressBatchSettled(one, "deflate64-raw", { outCapacity: 64, restartPoints: "scan" }), type, "deflate64-raw: a TypeError");
  for (const restartPoints of ["Scan", "scan ", "", "index"])
    await rejects(api.decompressBatchDetailed(one, "deflate", { outCapacity: 64, restartPoints }), type,
                  JSON.stringify(restartPoints) + ": a TypeError");
}

// x compressed by node's zlib with a full flush at every position of `at`
function flushed(x, at, format) {
  const mk = { "deflate-raw": zlib.createDeflateRaw, deflate: zlib.createDeflate, gzip: zlib.createGzip }[format];
  return new Promise((resolve, reject) => {
    const z = mk({ level: 6 });
    const chunks = [];
    z.on("data", (c) => chunks.push(c));
    z.on("error", reject);
    z.on("end", () => resolve(new Uint8Array(Buffer.concat(chunks))));
    const step = (k, from) => {
      if (k === at.length) return z.end(Buffer.from(x.subarray(from)));
      z.write(Buffer.from(x.subarray(from, at[k])));
      z.flush(zlib.constants.Z_FULL_FLUSH, () => step(k + 1, at[k]));
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
    const srcs = [x, x.subarray(0, 100), x.subarray(0, 3), x.subarray(0, 5000)];
    const ins = [await flushed(x, [65536, 70001], format), await flushed(srcs[1], [4, 8], format),
                 await flushed(srcs[2], [0, 1, 3], format), await flushed(srcs[3], [], format)];
    const options = { outCapacity: [150000, 100, 3, 5000], restartPoints: "scan" };
    const outs = await api.decompressBatch(ins, format, options);
    outs.forEach((o, i) => expect(same(o, srcs[i]), `${format}: input ${i} from the points the engine found`));
    const d = await api.decompressBatchDetailed(ins, format, options);
    expect(d.consumed[0] === ins[0].length && d.status[0] === 1, format + ": the whole stream is consumed");
    // a truncated stream fails alone, by status and message
    const cut = [ins[0], ins[1].subarray(0, ins[1].length - 12), ins[2], ins[3]];
    const s = await api.decompressBatchSettled(cut, format, options);
    expect(s[0].status === "fulfilled" && same(s[0].value, x), format + ": the neighbour of a broken stream");
    expect(s[1].status === "rejected" && s[1].reason.message === "process error: -3" &&
           s[1].reason.zmsg === "restart points do not decode the stream", format + ": the one failure");
    expect(s[2].status === "fulfilled" && same(s[2].value, srcs[2]), format + ": the stream behind it");
    // one byte short: the capacity outcome
    const short = await api.decompressBatchSettled([ins[3]], format, { outCapacity: 4999, restartPoints: "scan" });
    expect(short[0].status === "rejected" && short[0].reason.zmsg === "output capacity exceeded", format + ": capacity");
  }
  console.log("ok " + checks);
}

main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
