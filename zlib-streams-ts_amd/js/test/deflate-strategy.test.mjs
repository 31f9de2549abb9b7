// Compression strategies through the JavaScript host path (streams-api.mjs -> zsnapi.node
// -> zs_pool_deflate_batch_strategy): compressBatch*(inputs, format, {level, strategy}),
// one golden of tests/golden/deflate_strategy.json (C zlib 1.2.11) per strategy, the
// outputs read back through node's own zlib, and the rejection rules.
//   node deflate-strategy.test.mjs cpu   -- the argument checks only (no GPU needed)
import crypto from "crypto";
import fs from "fs";
import zlib from "zlib";

import * as corpus from "../../../tests/golden/corpus.mjs";
import * as api from "../streams-api.mjs";

let checks = 0;
const expect = (c, m) => { if (!c) throw new Error("FAIL " + m); checks++; };
const same = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.length), Buffer.from(b.buffer, b.byteOffset, b.length)) === 0;
const digest = (b) => [b.length, crypto.createHash("sha256").update(b).digest("hex").slice(0, 16)];

async function rejects(p, pred, what) {
  let e = null;
  try { await p; } catch (x) { e = x; }
  expect(e !== null && pred(e), what + (e ? ": " + e.message : ": no error"));
}

async function argumentChecks() {
  const one = [new Uint8Array([1, 2, 3])];
  const dict = new Uint8Array([1, 2, 3, 4]);
  expect([api.Z_DEFAULT_STRATEGY, api.Z_FILTERED, api.Z_HUFFMAN_ONLY, api.Z_RLE, api.Z_FIXED].join() === "0,1,2,3,4", "constants");
  for (const bad of [-1, 5, 1000]) {
    // deflateInit2_'s Z_STREAM_ERROR (deflate.ts:289-290), refused before any device is touched
    await rejects(api.compressBatch(one, "deflate-raw", { strategy: bad }), (e) => e.message === "init failed: -2",
                  "strategy " + bad + " is init failed: -2");
    await rejects(api.compressBatchSettled(one, "gzip", { strategy: bad }), (e) => e.message === "init failed: -2",
                  "settled: strategy " + bad);
    await rejects(api.compressBatchDetailed(one, "deflate", { strategy: bad }), (e) => e.code === "-2", "detailed: code -2");
  }
  for (const strategy of [1, 2, 3, 4]) {
    await rejects(api.compressBatch(one, "deflate-raw", { strategy, dictionary: dict }), (e) => e instanceof TypeError,
                  "strategy " + strategy + " with a dictionary is a TypeError");
    await rejects(api.compressBatchDetailed(one, "deflate", { strategy, dictionary: [dict] }), (e) => e instanceof TypeError,
                  "the detailed entry checks it too");
  }
}

const repeat = (byte, n) => new Uint8Array(n).fill(byte);
const concat = (...parts) => new Uint8Array(Buffer.concat(parts.map((p) => Buffer.from(p.buffer, p.byteOffset, p.length))));
const ascii = (s) => new Uint8Array(Buffer.from(s, "latin1"));

async function main() {
  await argumentChecks();
  if (process.argv[2] === "cpu") {
    console.log("ok " + checks);
    return;
  }
  const golden = JSON.parse(fs.readFileSync(new URL("../../../tests/golden/deflate_strategy.json", import.meta.url)));
  const text = (k, n) => corpus.text(corpus.streamSeed(k), n);
  // [golden, input, format, level, strategy] -- the inputs of tests/strategycases.py
  const cases = [
    ["filtered/deflate-raw/l6/T4096", text(4300, 4096), "deflate-raw", 6, api.Z_FILTERED],
    ["huff/gzip/l9/text16384", text(4006, 16384), "gzip", 9, api.Z_HUFFMAN_ONLY],
    ["huff/deflate/l6/text3", text(4003, 3), "deflate", 6, api.Z_HUFFMAN_ONLY],
    // Z_RLE as the reference runs it (the pool's contexts keep rle_ref = 1)
    ["rle/deflate-raw/l6/run519/ref1", concat(ascii("xy"), repeat(122, 519), ascii("pq")), "deflate-raw", 6, api.Z_RLE],
    ["fixed/deflate-raw/l4/text20000", text(4400, 20000), "deflate-raw", 4, api.Z_FIXED],
    ["fixed/gzip/l6/zeros20000", new Uint8Array(20000), "gzip", 6, api.Z_FIXED],
  ];
  const inflate = { "deflate-raw": zlib.inflateRawSync, deflate: zlib.inflateSync, gzip: zlib.gunzipSync };
  for (const [name, x, format, level, strategy] of cases) {
    expect(golden[name] !== undefined, "golden " + name);
    const inputs = [x, new Uint8Array(0), x.subarray(0, x.length >> 1), x];
    const outs = await api.compressBatch(inputs, format, { level, strategy });
    expect(JSON.stringify(digest(outs[0])) === JSON.stringify(golden[name]), name + ": zlib 1.2.11's bytes");
    expect(same(outs[0], outs[3]), name + ": the same input twice");
    outs.forEach((o, i) => expect(same(new Uint8Array(inflate[format](o)), inputs[i]), `${name}: node's zlib, input ${i}`));
    const back = await api.decompressBatch(outs, format);
    back.forEach((o, i) => expect(same(o, inputs[i]), `${name}: the engine's inflate, input ${i}`));
    const det = await api.compressBatchDetailed(inputs, format, { level, strategy });
    det.outputs.forEach((o, i) => expect(det.status[i] === 1 && same(o, outs[i]), `${name}: detailed, input ${i}`));
    const settled = await api.compressBatchSettled(inputs, format, { level, strategy });
    settled.forEach((s, i) => expect(s.status === "fulfilled" && same(s.value, outs[i]), `${name}: settled, input ${i}`));
  }
  // a strategy that is not a number means 0, and 0 is the plain call
  const x = text(4300, 4096);
  const plain = await api.compressBatch([x], "deflate", { level: 6 });
  for (const strategy of [undefined, null, "2", {}, 0])
    expect(same((await api.compressBatch([x], "deflate", { level: 6, strategy }))[0], plain[0]), "strategy " + String(strategy) + " is 0");
  expect(!same((await api.compressBatch([x], "deflate", { level: 6, strategy: 2 }))[0], plain[0]), "strategy 2 is not");
  // an invalid level with a strategy: as without
  await rejects(api.compressBatch([x], "deflate", { level: 10, strategy: 2 }), (e) => e.message === "init failed: -2", "level 10");
  console.log("ok " + checks);
}

main().catch((e) => { console.error(e); process.exit(1); });
