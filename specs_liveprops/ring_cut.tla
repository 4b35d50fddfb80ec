------------------------------ MODULE ring_cut ------------------------------
(* Written to show: THE KERNELS AT SIZE (specs_liveness/ring.tla's shape).  A fair counter cycles modulo N until an unfair process stops it, which it can do at c = Half - 1 only.  Q is c = 0 \/ c = Half: the ~Q subgraph cuts the ring into two arcs, chains of one-state components that the component search has to peel and the reach pass has to walk.  The first arc ends where the stopper can act; once stopped, the counter finishes and the behaviour stutters in a ~Q state: []<>Q is VIOLATED, the witness is c = 1 and the way from it to the final state is about Half steps long.  The second arc reaches that state through c = 0 only: none of its states is a bad start. *)
EXTENDS Naturals
CONSTANTS N, Half
(* --algorithm ring_cut
variables c = 0, stop = 0;

fair process Counter = 0
begin
  C: while stop = 0 do
       c := (c + 1) % N;
     end while;
end process

process Stopper = 1
begin
  S: await c = Half - 1;
     stop := 1;
end process

end algorithm *)

Cut == []<>(c = 0 \/ c = Half)
=============================================================================
